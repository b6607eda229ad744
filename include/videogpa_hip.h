/* videogpa_hip.h -- C ABI of libvgpa_hip.so: the MI355X (gfx950) kernels behind the VideoGPA DPO hot path.
 *
 * Boundary contract: plain pointers and sizes, no torch types; the CALLER owns every buffer
 * (outputs and workspaces); every call is asynchronous on `stream`, re-entrant, holds no global state; returns
 * 0 on success or a negative VGPA_ERR_* code and never throws.  One process per GPU.
 *
 * The reference (Hongyang-Du/VideoGPA) is pure Python and reaches these computations through PyTorch / diffusers /
 * PEFT objects; each entry point below cites the reference interface (file:line) it stands behind.  The Python
 * host side that mirrors those object APIs is `videogpa_amd/` (ctypes binding: videogpa_amd/_lib.py; the binding a
 * reference maintainer would add is shown in INTEGRATION.md).
 *
 * dtype codes: 0 = float32, 1 = bfloat16.  "BHS strides" = int64[3] element strides {batch, head, token} of a
 * [B, H, S, 64] bf16 view whose last dimension is contiguous (multiples of 8; base pointers 16-byte aligned).
 */
#ifndef VIDEOGPA_HIP_H
#define VIDEOGPA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* vgpa_stream_t; /* == hipStream_t */

#define VGPA_OK 0
#define VGPA_ERR_INVALID (-1)
#define VGPA_ERR_LAUNCH (-2)
#define VGPA_ERR_WORKSPACE (-3)

/* ---- Diffusion-DPO loss: train/loss.py:53-121 (DPOLoss.forward) + its autograd backward -------------------------
 * Each input is [B, N] with its own per-sample stride (paired layout [B,2,N]: win = base, lose = base + N, stride 2N).
 * out5 = {loss, reward_margin, winner_reward, loser_reward, accuracy}; dlogit[B] = dloss/dlogit_b (kept for bwd);
 * errs[B,4] = {e_win, e_lose, e_win_ref, e_lose_ref} (may be NULL).  loss_type 0 = sigmoid (label_smoothing
 * honoured), 1 = hinge.  flags bit0: round (v - tgt) to bf16 before squaring (what bf16 autocast does upstream). */
size_t vgpa_dpo_loss_workspace_bytes(int64_t B);
int32_t vgpa_dpo_loss_fwd(const void* v_win, const void* v_lose, const void* v_win_ref, const void* v_lose_ref,
                          const void* tgt_win, const void* tgt_lose, int64_t B, int64_t N, int64_t stride_pred,
                          int64_t stride_ref, int64_t stride_tgt, int32_t dtype, float beta, float label_smoothing,
                          int32_t loss_type, int32_t flags, float* out5, float* dlogit, float* errs, void* workspace,
                          size_t ws_bytes, vgpa_stream_t stream);
int32_t vgpa_dpo_loss_bwd(const void* v_win, const void* v_lose, const void* tgt_win, const void* tgt_lose, int64_t B,
                          int64_t N, int64_t stride_pred, int64_t stride_tgt, int64_t stride_grad, int32_t dtype, float beta,
                          int32_t flags, const float* dlogit, const float* grad_out, void* grad_win, void* grad_lose,
                          vgpa_stream_t stream);

/* ---- noising + v-targets: scheduler.add_noise / get_velocity, train/CogVideoX-5B/03_train.py:129-130,154-155 ------
 * x_pair [B,2,N], noise [B,N] shared by the pair, t [B]; tables = sqrt(abar), sqrt(1-abar) (fp32 [T]). */
int32_t vgpa_noise_velocity_paired(const void* x_pair, const void* noise, const int64_t* t, const float* sqrt_abar,
                                   const float* sqrt_1m_abar, int64_t B, int64_t N, int32_t num_train_timesteps,
                                   int32_t dtype, void* x_noisy_pair, void* v_target_pair, vgpa_stream_t stream);

/* flow-matching variant (train/Wan2.2-TI2V-5B/03_train.py:103-116): x_t = (1-sigma) x + sigma eps (fp32 when xt_f32, as
 * torch's promotion gives), v = eps - x; sigma fp32 [B]. */
int32_t vgpa_flow_noise_velocity_paired(const void* x_pair, const void* noise, const float* sigma, int64_t B, int64_t N,
                                        int32_t dtype, int32_t xt_f32, void* x_noisy_pair, void* v_target_pair,
                                        vgpa_stream_t stream);

/* ---- AdaLN-Zero pieces of CogVideoXBlock (diffusers CogVideoXLayerNormZero / AdaLayerNorm / LayerNorm), reached
 * from train/CogVideoX-5B/03_train.py:134-151.  x, out, dy, dx: bf16 [B,S,D], text tokens first (rows < text_len).
 * Per-range fp32 vectors [B,D] with a common batch stride; all four modulation pointers NULL = plain LayerNorm. */
int32_t vgpa_ln_modulate_fwd(const void* x, const float* ln_w, const float* ln_b, const float* shift_v,
                             const float* scale1p_v, const float* shift_t, const float* scale1p_t, int64_t mod_stride,
                             int64_t B, int64_t S, int64_t D, int64_t text_len, float eps, void* out, float* mean,
                             float* rstd, vgpa_stream_t stream);
int32_t vgpa_ln_modulate_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* ln_w,
                             const float* scale1p_v, const float* scale1p_t, int64_t mod_stride, int64_t B, int64_t S,
                             int64_t D, int64_t text_len, const void* dres, void* dx, vgpa_stream_t stream);
/* fused gated residual + following LN-modulate (the pair diffusers runs as `hidden += gate * out` then `norm(hidden)`):
 *   fwd: x_new = x + gate[range]*y ; n = LN(x_new) * (w (1+scale)) + (b (1+scale) + shift)      (y NULL: n = LN-mod(x) only)
 *   bwd: dx = dres + LN'(dn) ; dy = gate[range]*dx                                               (dres / dy may be NULL) */
int32_t vgpa_residual_ln_fwd(const void* x, const void* y, const float* gate_v, const float* gate_t, int64_t gate_stride,
                             const float* ln_w, const float* ln_b, const float* shift_v, const float* scale1p_v,
                             const float* shift_t, const float* scale1p_t, int64_t mod_stride, int64_t B, int64_t S, int64_t D,
                             int64_t text_len, float eps, void* x_new, void* n_out,
                             int64_t n_stride /* row stride of n_out in elements, >= D: n may be the head of a wider [rows, D+R]
                                                 buffer whose tail carries LoRA down-projections */,
                             float* mean, float* rstd, vgpa_stream_t stream);
int32_t vgpa_residual_ln_bwd(const void* dn, const void* x_new, const float* mean, const float* rstd, const float* ln_w,
                             const float* scale1p_v, const float* scale1p_t, int64_t mod_stride, const float* gate_v,
                             const float* gate_t, int64_t gate_stride, const void* dres, int64_t B, int64_t S, int64_t D,
                             int64_t text_len, void* dx, void* dy, int64_t dy_stride /* row stride of dy, >= D */,
                             vgpa_stream_t stream);
/* the same two passes with the result that feeds a frozen fp8 GEMM written ONLY as its e4m3 operand (no bf16 copy reaches memory):
 *   fwd_q8: n  -> q8 [B*S, D] bytes + q8_scale [B*S] fp32;   bwd_q8: dy = bf16(gate*dx) -> dy_q8 [B*S, D] bytes + dy_scale [B*S] fp32 (both required)
 * scale = rowmax / 448 (1 for an all-zero row), q = e4m3(bf16 value / scale), RNE, saturating: the bits of the bf16 entry followed by
 * vgpa_quant_fp8_rows.  x_new / mean / rstd / dx exactly as the bf16 entries write them; D % 8 == 0, D <= 4096. */
int32_t vgpa_residual_ln_fwd_q8(const void* x, const void* y, const float* gate_v, const float* gate_t, int64_t gate_stride,
                                const float* ln_w, const float* ln_b, const float* shift_v, const float* scale1p_v,
                                const float* shift_t, const float* scale1p_t, int64_t mod_stride, int64_t B, int64_t S, int64_t D,
                                int64_t text_len, float eps, void* x_new, void* q8, float* q8_scale, float* mean, float* rstd,
                                vgpa_stream_t stream);
int32_t vgpa_residual_ln_bwd_q8(const void* dn, const void* x_new, const float* mean, const float* rstd, const float* ln_w,
                                const float* scale1p_v, const float* scale1p_t, int64_t mod_stride, const float* gate_v,
                                const float* gate_t, int64_t gate_stride, const void* dres, int64_t B, int64_t S, int64_t D,
                                int64_t text_len, void* dx, void* dy_q8, float* dy_scale, vgpa_stream_t stream);
/* out = x + gate[range] * y (x NULL: out = gate * y, the backward of the y branch) */
int32_t vgpa_gate_residual(const void* x, const void* y, const float* gate_v, const float* gate_t, int64_t mod_stride,
                           int64_t B, int64_t S, int64_t D, int64_t text_len, void* out, vgpa_stream_t stream);
/* FeedForward activation "gelu-approximate" (tanh), bf16, n elements */
int32_t vgpa_gelu_tanh_fwd(const void* u, int64_t n, void* out, vgpa_stream_t stream);
int32_t vgpa_gelu_tanh_bwd(const void* u, const void* dy, int64_t n, void* du, vgpa_stream_t stream);

/* ---- QK-norm (LayerNorm over head_dim 64) + 3D RoPE (attn.norm_q/norm_k, apply_rotary_emb in
 * CogVideoXAttnProcessor2_0; RoPE only when image_rotary_emb is given: generate/CogVideoX-5B.py:72-77).
 * rope_cos/rope_sin: fp32 [S - text_len, 64] or NULL.  q_out is additionally multiplied by q_out_scale (the attention
 * kernels take q pre-multiplied by scale*log2(e)); the backward returns d/d(q_in) for the UNscaled normalised query. */
int32_t vgpa_qknorm_rope_fwd(const void* q_in, const void* k_in, void* q_out, void* k_out, const int64_t* qin_strides,
                             const int64_t* kin_strides, const int64_t* qout_strides, const int64_t* kout_strides,
                             const float* wq, const float* bq, const float* wk, const float* bk, const float* rope_cos,
                             const float* rope_sin, int64_t text_len, int64_t B, int64_t H, int64_t S, int64_t head_dim,
                             float eps, float q_out_scale, int32_t rope_mode, vgpa_stream_t stream);
int32_t vgpa_qknorm_rope_bwd(const void* dq_out, const void* dk_out, const void* q_in, const void* k_in, void* dq_in,
                             void* dk_in, const int64_t* dqout_strides, const int64_t* dkout_strides,
                             const int64_t* qin_strides, const int64_t* kin_strides, const int64_t* dqin_strides,
                             const int64_t* dkin_strides, const float* wq, const float* wk, const float* rope_cos,
                             const float* rope_sin, int64_t text_len, int64_t B, int64_t H, int64_t S, int64_t head_dim,
                             float eps, int32_t rope_mode, vgpa_stream_t stream);

/* ---- 3D full attention, non-causal, head_dim 64 (F.scaled_dot_product_attention in the same processor) ----------
 * CONTRACT: q is PRE-MULTIPLIED by scale*log2(e) in every entry point below; dq is the gradient w.r.t. the unscaled q.
 * lse2 = log2 sum_k exp2(q.k), fp32 [B,H,S]; delta = rowsum(dO * O), fp32 [B,H,S]. */
/* All tensors are bf16 views [B,H,S,64] given by ELEMENT strides {batch, head, token} (last dim contiguous, strides multiples of 8, base
 * pointers 16-byte aligned); `scale` is the softmax scale (dQ / dK multipliers).  The kernels are the "w1" structure of attention_w1.hip: one wave
 * per SIMD, 512-register waves, LDS-DMA ring, hand-scheduled main loops.
 * split_mode, in every call that takes one: when the number of (head, 256-row strip) tasks leaves a mostly empty last scheduling round on the
 * device, those leftover tasks are cut into chunks along the streamed axis (second small launch + fp32 merge) instead, the partial results going
 * through the caller-owned workspace.  -1 automatic, 0 never, k >= 2 force k chunks for every task (a short workspace is then VGPA_ERR_WORKSPACE). */
/* Backward, step 1: delta = rowsum(dO o O), of the output as the forward's residual tensor completes it (o_res / res_kind as
 * vgpa_attn_fwd_w1_res wrote them; o_res may be NULL: from o alone).  delta stands for rowsum(P o dP), which equals rowsum(dO o O) for the UNROUNDED O only; from the bf16 O alone (what flash-attention
 * backwards, torch's included, do) every row's dS stops summing to zero and dQ picks up a coherent error. */
int32_t vgpa_attn_bwd_delta_res(const void* o, const void* o_res, int32_t res_kind, const void* d_o, const int64_t* o_strides, const int64_t* ores_strides,
                                const int64_t* do_strides, float* delta, int64_t B, int64_t H, int64_t S, int64_t head_dim,
                                vgpa_stream_t stream);
/* Backward, step 3: dQ from lse2 / delta.  workspace: NULL (a single launch), or caller-owned with >= vgpa_attn_bwd_split_workspace_bytes (it may
 * be the one vgpa_attn_bwd_dkv_w1 used: the two calls run one after the other on a stream). */
size_t vgpa_attn_bwd_split_workspace_bytes(int64_t B, int64_t H, int64_t S);
int32_t vgpa_attn_bwd_dq_w1(const void* q, const void* k, const void* v, const void* d_o, const float* lse2, const float* delta,
                            void* dq, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                            const int64_t* do_strides, const int64_t* dq_strides, int64_t B, int64_t H, int64_t S, int64_t head_dim,
                            float scale, int32_t split_mode, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* The forward: o = softmax(q k^T) v and lse2.  The workspace (>= vgpa_attn_fwd_w1_workspace_bytes) is required.  Scores are shifted per row by M' = min(b, m_s + 64), b = the bound |q| max|k|, m_s = the row's maximum
 * over 64 keys spread evenly over the sequence, instead of a running maximum; 256-row strips whose sum overflows or comes too close to underflow (a row whose true
 * maximum lies > ~176 log2 units above the sampled one) are redone by the online-softmax kernel in the same call.  lse2 is formed from the sum of the bf16-ROUNDED
 * weights (the ones the PV product multiplies: O is an exact convex combination of V rows); it differs from the exact value by a row's weighted mean rounding error
 * (<= 2^-8 relative, i.e. 5.6e-3 in log2 units, on a one-hot row; ~ 2e-3 / sqrt(n) on a row spread over n keys: tests/attn_tol.py). */
size_t vgpa_attn_fwd_w1_workspace_bytes(int64_t B, int64_t H, int64_t S);
/* It also writes what the bf16 rounding of the output dropped ([B,H,S,64] view o_res with its own ELEMENT strides; NULL = not
 * written), for the backward's delta (vgpa_attn_bwd_prep_w1_res / vgpa_attn_bwd_delta_res).  res_kind:
 *   VGPA_RES_BF16 (1)  bf16 elements: O_fp32 - bf16(O);
 *   VGPA_RES_8    (2)  uint8 elements: eight further mantissa bits, 128 + clamp(rint((O_fp32 - bf16(O)) * 2^8 / ulp(bf16(O))), -128, 127).
 * Either way (o, o_res) carries the output to 2^-17 relative; the 8-bit form costs half the bytes (1 per output element). */
#define VGPA_RES_NONE 0
#define VGPA_RES_BF16 1
#define VGPA_RES_8 2
int32_t vgpa_attn_fwd_w1_res(const void* q, const void* k, const void* v, void* o, void* o_res, int32_t res_kind, float* lse2, const int64_t* q_strides,
                             const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides, const int64_t* ores_strides,
                             int64_t B, int64_t H, int64_t S, int64_t head_dim, float scale, int32_t split_mode, void* workspace,
                             size_t ws_bytes, vgpa_stream_t stream);
/* Redo accounting of vgpa_attn_fwd_w1_res: after the call the workspace holds, behind its first B*H uint32 words (max_k |k|^2 per head), one int32 per
 * (batch, head, 256-row strip): non-zero = the strip held a row outside what the shifted loop represents (see above) and it was redone by the online-softmax kernel inside the same call.  Results never depend on it; time does.
 * vgpa_attn_fwd_online_res: same arguments, results and workspace, EVERY strip on the online-softmax kernel -- the faster call when most strips would be flagged
 * (one sweep instead of two).  The host side (transformer.AttentionCore) reads the count on a layer's first calls and switches that layer. */
int32_t vgpa_attn_fwd_online_res(const void* q, const void* k, const void* v, void* o, void* o_res, int32_t res_kind, float* lse2, const int64_t* q_strides,
                                 const int64_t* k_strides, const int64_t* v_strides, const int64_t* o_strides, const int64_t* ores_strides,
                                 int64_t B, int64_t H, int64_t S, int64_t head_dim, float scale, int32_t split_mode, void* workspace,
                                 size_t ws_bytes, vgpa_stream_t stream);
/* w1 backward, step 1 and step 2: vgpa_attn_bwd_prep_w1_res writes delta (fp32 [B,H,S], as vgpa_attn_bwd_delta_res; o_res may be NULL) and the
 * statistics planes stats = fp32 [B,H,2,S] = {-lse2, -delta}; vgpa_attn_bwd_dkv_w1 writes dK, dV from `stats`; its workspace as in
 * vgpa_attn_bwd_dq_w1 (NULL: a single launch). */
int32_t vgpa_attn_bwd_prep_w1_res(const void* o, const void* o_res, int32_t res_kind, const void* d_o, const float* lse2, const int64_t* o_strides,
                                  const int64_t* ores_strides, const int64_t* do_strides, float* delta, float* stats, int64_t B, int64_t H,
                                  int64_t S, int64_t head_dim, vgpa_stream_t stream);
int32_t vgpa_attn_bwd_dkv_w1(const void* q, const void* k, const void* v, const void* d_o, const float* stats, void* dk, void* dv,
                             const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides, const int64_t* do_strides,
                             const int64_t* dk_strides, const int64_t* dv_strides, int64_t B, int64_t H, int64_t S, int64_t head_dim,
                             float scale, int32_t split_mode, void* workspace, size_t ws_bytes, vgpa_stream_t stream);

/* ---- LoRA A.B contractions (peft Linear.forward `lora_B(lora_A(x)) * scaling` and its backward for the adapters of
 * train/CogVideoX-5B/03_train.py:102-106).  bf16 row-major operands with explicit row strides (elements).
 *   down  : T[M,R]  = X[M,K] A[R,K]^T                     K % 64 == 0, R <= 256
 *   up_add: Y[M,N]  = (accumulate ? Y : 0) + s * T[M,rp] Bw[N,rp]^T   rp in {16,32,48,64,96,128,192}, N % 8 == 0
 *   grad  : G[P,Q]  = s * U[M,P]^T V[M,Q]                 G fp32, overwritten; P % 8 == 0, Q % 8 == 0
 * Every row stride is a multiple of 8 and at least the row's length (ldx >= K, ldt >= R resp. rp, ldy >= N, ldb >= rp, ldu >= P, ldv >= Q, ldg >= Q): rows that
 * overlap, or run backwards, are VGPA_ERR_INVALID.  Operands that are read are 16-byte aligned, T of `down` 8-byte (it is stored in 8-byte pieces), Y 16-byte. */
int32_t vgpa_lora_down(const void* X, int64_t ldx, const void* A, void* T, int64_t ldt, int64_t M, int64_t K, int64_t R,
                       vgpa_stream_t stream);
int32_t vgpa_lora_up_add(void* Y, int64_t ldy, const void* T, int64_t ldt, const void* Bw, int64_t ldb, float s, int64_t M,
                         int64_t N, int64_t rp, int32_t accumulate, vgpa_stream_t stream);
/* grad is bit-reproducible: per-row-range partials in the caller's workspace (>= vgpa_lora_grad_workspace_bytes) + an ordered merge */
size_t vgpa_lora_grad_workspace_bytes(int64_t M, int64_t P, int64_t Q);
int32_t vgpa_lora_grad_ws(const void* U, int64_t ldu, const void* V, int64_t ldv, float* G, int64_t ldg, float s, int64_t M,
                          int64_t P, int64_t Q, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* adapter refresh of the K-extended projection operands after an optimizer step (PEFT re-reads lora_A / lora_B in every forward,
 * peft/tuners/lora/layer.py Linear.forward; here the extended GEMM operands cache them): a = bf16(A[r, K]), sB = bf16(float(bf16(B[Dn, r])) * s)
 * -> a_cat [r, K], wt_tail[k * ld_wt + rr] = a (the [K, N + R] operand's tail columns), w_tail[n * ld_w + rr] = sB (the [N, K + R] operand's
 * tail columns), sbt [rr * Dn + n] = sB.  A, B fp32 contiguous, outputs bf16. */
int32_t vgpa_lora_ext_refresh(const float* A, const float* B, float s, int64_t r, int64_t K, int64_t Dn, void* a_cat, void* wt_tail, int64_t ld_wt,
                              void* w_tail, int64_t ld_w, void* sbt, vgpa_stream_t stream);

/* ---- feed-forward GEMM with fused epilogue: diffusers FeedForward(activation_fn="gelu-approximate") inside CogVideoXBlock
 * (the reference reaches it through diffusers cogvideox_transformer_3d.py; train/CogVideoX-5B/utils.py:255-289 drives the blocks).
 * C[M, N] = epi(X[M, K] W[N, K]^T + bias[N]), bf16 in / fp32 accumulate / bf16 out; N % 128 == 0, K % 64 == 0, ld* in elements.
 *   epilogue 0: identity   1: gelu_tanh (aux != NULL: the bf16 pre-activation is also stored to aux)   2: C = acc * gelu_tanh'(aux) */
#ifdef VGPA_VARIANTS   /* probe: profiles/r03_gemm_probe.txt */
int32_t vgpa_gemm_bf16(const void* X, int64_t ldx, const void* W, int64_t ldw, const void* bias, void* C, int64_t ldc, void* aux,
                       int64_t ldaux, int32_t M, int32_t N, int32_t K, int32_t epilogue, vgpa_stream_t stream);
#endif

/* ---- head_dim-128 attention with separate query / key lengths: the self- and cross-attention of the Wan2.2-TI2V-5B denoiser
 * (train/Wan2.2-TI2V-5B/03_train.py:150-163; WanModel comes from the un-vendored Wan2.2 checkout: 24 heads x 128, text length 512).
 * q, o, d_o, dq: [B, H, Sq, 128] views; k, v, dk, dv: [B, H, Skv, 128] views; *_strides = element strides {batch, head, token},
 * last dim contiguous.  lse2 [B, H, Sq] fp32 = log2-domain log-sum-exp written by the forward. */
/* With a workspace (vgpa_attn128_fwd_workspace_bytes) and Skv >= 1024 the forward runs on the one-wave-per-SIMD / LDS-DMA structure
 * (row-bound softmax shift, flagged strips redone with a running max); workspace NULL: the compiler-scheduled kernel. */
size_t vgpa_attn128_fwd_workspace_bytes(int64_t B, int64_t H, int64_t Sq);
/* o_res8 (optional; uint8 [B, H, Sq, 128] view with its own element strides, NULL = not written): eight further mantissa bits of every output value
 * (VGPA_RES_8 of vgpa_attn_fwd_w1_res) for the backward's delta = rowsum(dO o O) -- pass the same tensor to vgpa_attn128_bwd. */
int32_t vgpa_attn128_fwd(const void* q, const void* k, const void* v, void* o, float* lse2, const int64_t* q_strides, const int64_t* k_strides,
                         const int64_t* v_strides, const int64_t* o_strides, void* o_res8, const int64_t* ores_strides, int64_t B, int64_t H,
                         int64_t Sq, int64_t Skv, float scale, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* The head_dim-128 forward on OCP-e4m3 matrix operands (BASELINE configs[4] "fp8 MFMA path"): q (with scale * log2 e folded in), k and v are quantised
 * with one power-of-two scale per (batch, head) and tensor, v transposed, by two prep kernels; both products run as v_mfma_scale_f32_32x32x64_f8f6f4
 * with the scales -- and a per-tile, per-row power of two for the softmax weights -- on the instruction's E8M0 operands; row sums and lse2 stay fp32.
 * Arguments and results as vgpa_attn128_fwd; the workspace (>= vgpa_attn128_fwd_f8_workspace_bytes, 256-byte aligned) is REQUIRED and is scratch.
 * The softmax shift of a row is M' = b - n, b = |q8 row| max|k8 row| and n = floor(max(0, b - (m_s + 64))) with m_s the row's maximum over 64 keys spread evenly
 * over the sweep (as vgpa_attn_fwd_w1_res; an INTEGER step off the bound, so the e4m3 bits of the weights do not depend on it); 256-row strips with a row it cannot
 * represent (row sum outside [2^-100, 2^118), M' > 1024, a non-finite accumulator) are redone by the bf16 running-max kernel inside the call.
 * Forward only.  q_deq / k_deq / v_deq (optional, all three or none; bf16 [B,H,S,128] views with their stride triples): the operands the products really ran
 * on, dequantised EXACTLY (an e4m3 value times a power of two is a bf16 number): k8 2^ek, v8 2^ev and q8 2^eq -- the query PRE-SCALED by scale * log2 e.
 * vgpa_attn128_bwd_prescaled run on THEM with this call's lse2, output and o_res8 is the straight-through gradient of this forward: its recomputed scores are
 * this call's bit for bit, its softmax weights this call's p / l (rows sum to one) and delta = rowsum(dO o O) matches them. */
size_t vgpa_attn128_fwd_f8_workspace_bytes(int64_t B, int64_t H, int64_t Sq, int64_t Skv);
int32_t vgpa_attn128_fwd_f8(const void* q, const void* k, const void* v, void* o, float* lse2, const int64_t* q_strides, const int64_t* k_strides,
                            const int64_t* v_strides, const int64_t* o_strides, void* o_res8, const int64_t* ores_strides, void* q_deq, void* k_deq,
                            void* v_deq, const int64_t* qd_strides, const int64_t* kd_strides, const int64_t* vd_strides, int64_t B, int64_t H,
                            int64_t Sq, int64_t Skv, float scale, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* workspace (vgpa_attn128_bwd_workspace_bytes): delta + the statistics planes.  dkv_mode -1 = automatic (w1 dK/dV kernel from 1024 queries on),
 * 0 = compiler-scheduled kernel, 1 = w1 kernel */
size_t vgpa_attn128_bwd_workspace_bytes(int64_t B, int64_t H, int64_t Sq);
int32_t vgpa_attn128_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse2, void* dq, void* dk,
                         void* dv, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                         const int64_t* o_strides, const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides,
                         const int64_t* dv_strides, const void* o_res8, const int64_t* ores_strides, int64_t B, int64_t H, int64_t Sq, int64_t Skv,
                         float scale, int32_t dkv_mode, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* vgpa_attn128_bwd for a query that arrives PRE-SCALED by scale * log2 e (q = vgpa_attn128_fwd_f8's q_deq; k = k_deq, v = v_deq): scores are q.k as they stand
 * (log2 units); dq = scale dS k is the gradient w.r.t. the UNscaled query, dk = ln 2 dS^T q (= scale dS^T q_unscaled).  Everything else as vgpa_attn128_bwd. */
int32_t vgpa_attn128_bwd_prescaled(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse2, void* dq, void* dk,
                                   void* dv, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                   const int64_t* o_strides, const int64_t* do_strides, const int64_t* dq_strides, const int64_t* dk_strides,
                                   const int64_t* dv_strides, const void* o_res8, const int64_t* ores_strides, int64_t B, int64_t H, int64_t Sq, int64_t Skv,
                                   float scale, int32_t dkv_mode, void* workspace, size_t ws_bytes, vgpa_stream_t stream);

/* ---- row kernels of the Wan2.2 denoiser block (WanAttentionBlock / WanRMSNorm / rope_apply of the Wan2.2 checkout imported at
 * train/Wan2.2-TI2V-5B/03_train.py:43-48).  fp32 residual stream, bf16 matmul operands.  Per-token modulation as a table: row
 * gid[row] of a [groups, mod_stride] fp32 table (shift / scale / gate point at their chunk's column offset); gid NULL = row 0.
 *   ln_mod_fwd : out(row stride out_ld >= D: the LoRA tail of the consuming projection may follow each row) = ([round_bf16] LN_eps(x)) * ln_w + ln_b,
 *                then * (1 + scale[g]) + shift[g]   (affine / modulation optional); with q8 / q8_scale the same rows are ALSO (or, out NULL, only) written
 *                as the e4m3 operand of the fp8 feed-forward GEMM: q8 [rows, D] bytes, q8_scale [rows] fp32, bit-identical to vgpa_quant_fp8_rows of the bf16
 *                output.  With y the row is first x_out(fp32) = x + y(bf16) * gate[g] (gate NULL = 1), the gated residual add in front of this LayerNorm
 *                (upstream WanAttentionBlock.forward: `x = x + y * e[2]` followed by norm3 / norm2 of that x), in the same pass.
 *   ln_mod_bwd : dx(fp32) = [dres +] LN-backward(dy (1 + scale) ln_w); with dy_prev also dy_prev(bf16, row stride ld_dy_prev) = dx * gate_prev[g] (NULL = 1),
 *                the gradient of the y of that residual add.  gate / gate_prev index the same table rows as shift / scale (mod_stride).
 *   dtypes (VGPA_DTYPE_*), each combination one kernel instantiation, anything else VGPA_ERR_INVALID:
 *                forward   x fp32 | bf16 -> bf16 out and / or q8;   x fp32 + y -> the same, round_xhat 0;   x fp32 -> fp32 out, no y / affine / q8 / round_xhat
 *                backward  dy bf16, x fp32 | bf16;   dy bf16, x fp32 + dy_prev;   dy fp32, x fp32, no dy_prev / ln_w / dres
 *                (the fp32 form is WanModel's output head: upstream Head.forward runs LN, modulation and the projection in fp32; reference call site
 *                train/Wan2.2-TI2V-5B/03_train.py:227-233 through WanModel.forward)
 *   gate_residual: out(fp32) = [x +] y(bf16) * gate[g]  (gate NULL = 1; out may alias x)
 *   gate_bwd   : dy(bf16, row stride ld_dy) = dout(fp32) * gate[g];   gate_bwd_q8: the same rows as e4m3 + per-row scale (fp8 dX GEMM operand)
 *   rms_rope   : n = bf16(u rsqrt(mean(u^2) + eps)) over the whole row [heads * head_dim]; y = bf16(n w); interleaved pairs of every head
 *                rotated by the angle at rope_{cos,sin}[(row % L) * head_dim/2 + pair]  (NULL: no rotation); u / out / dout / du are row-strided
 *                (ld_* in elements) so that q and k are read from and their gradients written into the fused [rows, 3 D (+ LoRA tail)] buffers */
int32_t vgpa_wan_ln_mod_fwd(const void* x, int32_t x_dtype, const void* y, const float* gate, float* x_out, const int32_t* gid, const float* ln_w,
                            const float* ln_b, const float* shift, const float* scale, int64_t mod_stride, int64_t rows, int64_t D, float eps,
                            int32_t round_xhat, void* out, int32_t out_dtype, int64_t out_ld, void* q8, float* q8_scale, float* mean, float* rstd,
                            vgpa_stream_t stream);
int32_t vgpa_wan_ln_mod_bwd(const void* dy, int32_t dy_dtype, const void* x, int32_t x_dtype, const float* mean, const float* rstd, const int32_t* gid,
                            const float* ln_w, const float* scale, int64_t mod_stride, int64_t rows, int64_t D, const float* dres, float* dx,
                            const float* gate_prev, void* dy_prev, int64_t ld_dy_prev, vgpa_stream_t stream);
int32_t vgpa_wan_gate_residual(const float* x, const void* y, const int32_t* gid, const float* gate, int64_t mod_stride, int64_t rows, int64_t D, float* out,
                               vgpa_stream_t stream);
int32_t vgpa_wan_gate_bwd(const float* dout, const int32_t* gid, const float* gate, int64_t mod_stride, int64_t rows, int64_t D, void* dy, int64_t ld_dy,
                          vgpa_stream_t stream);
int32_t vgpa_wan_gate_bwd_q8(const float* dout, const int32_t* gid, const float* gate, int64_t mod_stride, int64_t rows, int64_t D, void* q8,
                             float* q8_scale, vgpa_stream_t stream);
int32_t vgpa_wan_rms_rope_fwd(const void* u, int64_t ld_u, const void* w, const float* rope_cos, const float* rope_sin, int64_t L, int64_t head_dim,
                              int64_t rows, int64_t D, float eps, void* out, int64_t ld_out, float* rstd, vgpa_stream_t stream);
int32_t vgpa_wan_rms_rope_bwd(const void* dout, int64_t ld_dout, const void* u, int64_t ld_u, const float* rstd, const void* w, const float* rope_cos,
                              const float* rope_sin, int64_t L, int64_t head_dim, int64_t rows, int64_t D, void* du, int64_t ld_du, vgpa_stream_t stream);

/* ---- fp8 operand preparation for the frozen feed-forward GEMMs of the Wan2.2 path (BASELINE.json configs[4]: "fp8 MFMA path"):
 * per-row dynamic quantisation of bf16 rows to OCP e4m3: scale[m] = amax(row) / 448 (1 for a zero row), q = e4m3(x / scale), RNE, saturating.
 * x [M, K] bf16 with row stride ldx (elements); q [M, K] bytes, contiguous; scale [M] fp32. */
int32_t vgpa_quant_fp8_rows(const void* x, int64_t ldx, void* q, float* scale, int64_t M, int64_t K, vgpa_stream_t stream);
/* the feed-forward's activation written as that operand by its producer: q8 = e4m3(bf16(gelu_tanh(u)) / scale) resp. of bf16(dy * gelu_tanh'(u));
 * u / dy [rows, K] bf16 contiguous, K <= 16384; bit-identical to vgpa_gelu_tanh_{fwd,bwd} followed by vgpa_quant_fp8_rows */
int32_t vgpa_gelu_tanh_fwd_q8(const void* u, int64_t rows, int64_t K, void* q8, float* q8_scale, vgpa_stream_t stream);
int32_t vgpa_gelu_tanh_bwd_q8(const void* u, const void* dy, int64_t rows, int64_t K, void* q8, float* q8_scale, vgpa_stream_t stream);

/* ---- VGGT input preprocessing: utils/model_utils.py:16-85 preprocess_images_from_numpy (PIL bicubic resize to width 518 /
 * longer side 518, ToTensor, centre crop or white pad).  frames uint8 [T, H, W, 3] -> out float32 [T, 3, out_h, out_w].
 * mode 0 = "crop", 1 = "pad".  vgpa_preprocess_shape is host arithmetic only (:36-48, :54-71). */
int32_t vgpa_preprocess_shape(int32_t H, int32_t W, int32_t mode, int32_t* out_h, int32_t* out_w);
size_t vgpa_preprocess_workspace_bytes(int32_t T, int32_t H, int32_t W, int32_t mode);
int32_t vgpa_preprocess_frames(const void* frames, int32_t T, int32_t H, int32_t W, int32_t mode, float* out, void* workspace,
                               size_t ws_bytes, vgpa_stream_t stream);

/* PIL `Image.resize((out_w, out_h), filter)` of uint8 frames [T, H, W, 3] -> uint8 [T, out_h, out_w, 3], bit-exact with Pillow's 8-bit ImagingResample
 * (the same two passes as above).  filter 0 = BICUBIC, 1 = LANCZOS (sinc(x) sinc(x / 3), support 3).  generate/CogVideoX-5B-I2V.py -> diffusers
 * VaeImageProcessor.preprocess (Lanczos to 720 x 480); replicate.py:201 (bicubic first). */
size_t vgpa_image_resize_workspace_bytes(int32_t T, int32_t H, int32_t W, int32_t out_h, int32_t out_w, int32_t filter);
int32_t vgpa_image_resize(const void* frames, int32_t T, int32_t H, int32_t W, int32_t out_h, int32_t out_w, int32_t filter, void* out,
                          void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* uint8 [T, H, W, 3] -> [T, 3, H, W] (dtype 0 | 1) = x / 255 * 2 - 1, formed in fp32 in that order and rounded once */
int32_t vgpa_image_to_pm1(const void* image_u8, int64_t T, int64_t H, int64_t W, int32_t dtype, void* out, vgpa_stream_t stream);

/* ---- Depth Anything 3 input processing (depth_anything_3/utils/io/input_processor.py, api.py:_add_processed_images; csrc/da3_input.hip).
 * vgpa_da3_resize: cv2.resize of uint8 frames [T, H, W, 3] with OpenCV's 8-bit semantics restated (not pinned to a build: see the file header).
 *   mode 0 = INTER_AREA (out_h <= H and out_w <= W, VGPA_ERR_INVALID otherwise: nothing is launched), 1 = INTER_CUBIC (any size).
 *   Destination, exactly one of: out_u8 uint8 [T, out_h, out_w, 3] (x, processed, table NULL), or the last stage's pair as the resize's epilogue
 *   (out_u8 NULL): x fp32 [T, 3, out_h, out_w] = (u / 255 - mean) / std in torchvision's order and roundings, processed uint8 [T, out_h, out_w, 3]
 *   = table[c][u], table uint8 [3][256] on the device.  The workspace holds the tap tables (0 bytes on the integer-scale area path).
 * vgpa_da3_normalize: that last stage alone on the box (top, left, h, w) of image_u8 [T, H, W, 3]. */
size_t vgpa_da3_resize_workspace_bytes(int32_t H, int32_t W, int32_t out_h, int32_t out_w, int32_t mode);
int32_t vgpa_da3_resize(const void* frames, int32_t T, int32_t H, int32_t W, int32_t out_h, int32_t out_w, int32_t mode, void* out_u8, float* x,
                        void* processed, const void* table, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
int32_t vgpa_da3_normalize(const void* image_u8, int32_t T, int32_t H, int32_t W, int32_t top, int32_t left, int32_t h, int32_t w, float* x,
                           void* processed, const void* table, vgpa_stream_t stream);

/* ---- one sampler step of the generate loop: guidance + v-prediction + scheduler update + the next transformer input, one pass
 * (diffusers CogVideoXImageToVideoPipeline.__call__ loop body behind the transformer; generate/CogVideoX-5B-I2V.py:70-89).
 *   v = v_u + g (v_c - v_u) when `guided` (v is [2B, N] = [uncond | cond]), else v [B, N];   x0 = sa x - sb v;
 *   x_next = k_x x + k_0 x0 + k_old x0_old + k_n noise     (a NULL x0_old / noise leaves its term out)
 * N = F C hw.  v in v_dtype; x, noise, image_latents [B, F, C_img, hw], x_next and packed in dtype; x0_old and x0 (may be NULL) fp32.
 * packed (NULL with image_latents NULL): [packed_groups * B, F, C + C_img, hw], channels [0, C) = x_next, [C, C + C_img) = image_latents, for each
 * of the 1 | 2 groups.  C hw and C_img hw must be multiples of 8 (VGPA_ERR_INVALID otherwise, nothing is launched).  fp32 arithmetic without
 * contraction, one rounding at each store. */
int32_t vgpa_sampler_step(const void* v, int32_t v_dtype, int32_t guided, const void* x, const float* x0_old, const void* noise,
                          const void* image_latents, int64_t B, int64_t F, int64_t C, int64_t C_img, int64_t hw, int32_t dtype, float g,
                          float sa, float sb, float k_x, float k_0, float k_old, float k_n, void* x_next, float* x0, void* packed,
                          int32_t packed_groups, vgpa_stream_t stream);

/* ---- optimizer on one flat fp32 buffer of all LoRA parameters: gradient_clip_val=1.0 + torch.optim.AdamW,
 * train/CogVideoX-5B/03_train.py:208-213,266.  norm_out[0] = grad_scale * ||grad||_2. */
size_t vgpa_grad_norm_workspace_bytes(void);
int32_t vgpa_grad_norm(const float* grad, int64_t n, float grad_scale, float* norm_out, void* workspace, size_t ws_bytes,
                       vgpa_stream_t stream);
int32_t vgpa_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int64_t step, float grad_scale, float max_norm,
                        const float* total_norm, vgpa_stream_t stream);

/* ---- geometry-consistency scorer ---------------------------------------------------------------------------------
 * project_points: utils/projection_utils.py:12-51 (+ :57-101 batch loop and [-1,1] output) with the confidence filter
 * of utils/pointcloud_utils.py:47-73 as a per-point predicate.  pc/colors fp32 [N,3], conf fp32 [N] or NULL,
 * K fp32 [T,3,3], E fp32 [T,e_rows,4] (e_rows 3 or 4).  canvas u8 [T,H,W,3] and/or out_f fp32 [T,3,H,W]. */
size_t vgpa_project_points_workspace_bytes(int64_t T, int64_t H, int64_t W);
int32_t vgpa_project_points(const float* pc, const float* colors, const float* conf, float conf_thr,
                            const float* conf_thr_dev /* device fp32[1] or NULL: overrides conf_thr */, const float* K,
                            const float* E, int32_t e_rows, int64_t N, int64_t T, int64_t H, int64_t W, uint8_t* canvas,
                            float* out_f, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* compute_motion_score_vectorized, metrics/consistency_score.py:8-40 */
int32_t vgpa_motion_score(const float* E, int32_t e_rows, int64_t T, float* out, vgpa_stream_t stream);
/* kornia find_fundamental (8-point) + sampson_epipolar_distance as used by metrics/epipolar.py:197-213 */
int32_t vgpa_epipolar_sampson(const float* p1, const float* p2, const int64_t* offsets, int64_t n_pairs, float* err_out,
                              float* F_out, vgpa_stream_t stream);

/* Confidence cut of get_colored_pointcloud, utils/pointcloud_utils.py:44-73: thr_out[0] (device) = k-th largest valid
 * confidence, k = max(1, ceil(n_valid * (1 - conf_thres / 100))) in double, as the reference forms it from the Python float (a
 * float32 conf_thres moves k by one, e.g. 33.3 at n_valid = 1000); -inf for conf_thres <= 0 or no valid point.  On-device
 * radix select (replaces torch.topk + .item()). */
size_t vgpa_conf_threshold_workspace_bytes(void);
int32_t vgpa_conf_threshold(const float* conf, int64_t N, double conf_thres, float* thr_out, void* workspace, size_t ws_bytes,
                            vgpa_stream_t stream);
/* MSEMetric / PSNRMetric.compute incl. the bilinear-resize branch, metrics/mse.py:14-29,56-80: rep [T,C,H2,W2] is resized to
 * gt's [H,W] (F.interpolate bilinear, align_corners=False).  psnr 0: mse; 1: 10 log10(1/mse), 100 when mse == 0.
 * dtype 0 f32 / 2 u8; layout 0 [T,C,H,W] / 1 [T,H,W,C]; is_tensor selects the torch.Tensor vs numpy range heuristics
 * (metrics/mse.py:31-54). */
size_t vgpa_frame_metric_workspace_bytes(void);
int32_t vgpa_frame_metric(const void* gt, int32_t gt_dtype, int32_t gt_layout, int32_t gt_is_tensor, const void* rep,
                          int32_t rep_dtype, int32_t rep_layout, int32_t rep_is_tensor, int64_t T, int64_t C, int64_t H,
                          int64_t W, int64_t H2, int64_t W2, int32_t psnr, float* out, void* workspace, size_t ws_bytes,
                          vgpa_stream_t stream);
/* SSIMMetric.compute, metrics/mse.py:101-134 = piq.ssim(gt, rep, data_range=1.0) at piq's defaults (11 x 11 Gaussian window, sigma 1.5,
 * k1 0.01, k2 0.03, average pool by max(1, round_half_even(min(H, W) / 256)) unless downsample == 0).  gt and rep share [T,C,H,W]
 * (no resize; a pooled side below 11 is an invalid argument); dtype / layout / is_tensor as vgpa_frame_metric.  out_per_frame fp32 [T]
 * and / or out_mean fp32 [1] (either may be NULL).  Results are run-to-run bit-identical (fixed-order fp64 reduction, no float atomics). */
size_t vgpa_frame_ssim_workspace_bytes(int64_t T, int64_t C, int64_t H, int64_t W);
int32_t vgpa_frame_ssim(const void* gt, int32_t gt_dtype, int32_t gt_layout, int32_t gt_is_tensor, const void* rep, int32_t rep_dtype,
                        int32_t rep_layout, int32_t rep_is_tensor, int64_t T, int64_t C, int64_t H, int64_t W, int32_t downsample,
                        float* out_per_frame, float* out_mean, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* Input side of LPIPSMetric.compute, metrics/lpips.py:21-63 (the LPIPS network itself is the caller's): frames -> fp32
 * [T,C,Ho,Wo] in [-1,1] by the reference's range rules, bilinearly resized when (Ho,Wo) != (H,W). */
int32_t vgpa_frames_to_pm1(const void* src, int32_t dtype, int32_t layout, int32_t is_tensor, int64_t T, int64_t C, int64_t H,
                           int64_t W, int64_t Ho, int64_t Wo, float* out, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* MVCSMetric.compute, metrics/mvcs.py:12-114.  depth fp32 [T,H,W]; K fp32 [T,k_dim,k_dim] (k_dim 3|4); E fp32
 * [T,e_rows(3|4),4] world-to-camera; out[0] = exp(-mean over valid consecutive pairs of the masked depth MSE). */
size_t vgpa_mvcs_workspace_bytes(int64_t T);
int32_t vgpa_mvcs(const float* depth, const float* K, int32_t k_dim, const float* E, int32_t e_rows, int64_t T, int64_t H,
                  int64_t W, float* out, void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* DA3 world points, pipelines/process_video.py:151-156 (affine_inverse + unproject_depth,
 * depth_anything_3/utils/geometry.py:54-59,434-497).  depth fp32 [T,H,W], K fp32 [T,3,3], E fp32 [T,e_rows,4] -> world
 * fp32 [T,H,W,3]. */
int32_t vgpa_unproject_depth(const float* depth, const float* K, const float* E, int32_t e_rows, int64_t T, int64_t H,
                             int64_t W, float* world, vgpa_stream_t stream);
/* pose_encoding_to_extri_intri("absT_quaR_FoV"), vggt/utils/pose_enc.py:62-124: pe fp32 [n,9] -> ext fp32 [n,3,4],
 * intr fp32 [n,3,3] or NULL. */
int32_t vgpa_pose_decode(const float* pose_enc, int64_t n, float image_h, float image_w, float* ext, float* intr,
                         vgpa_stream_t stream);

/* ---- VGGT prediction heads: vggt/heads/dpt_head.py, camera_head.py (csrc/vggt_heads.hip) ---------------------------------
 * All fp32, channels-last (NHWC), forward only, 16-byte aligned bases.  The convolutions are implicit GEMMs on the exact-fp32
 * MFMA (v_mfma_f32_32x32x2_f32); Cin and Cout multiples of 16, H and W arbitrary.
 *
 * 3x3, pad 1, stride 1 | 2:  out = conv(relu?(x)) + bias? + relu?(res)? + res2?   (bias / res / res2 may be NULL; res, res2 and out
 * are [N,Ho,Wo,Cout], Ho = (H - 1) / stride + 1).  flags bit0: ReLU on the input, bit1: ReLU on `res` -- the reference's
 * ResidualConvUnit applies its in-place ReLU to the tensor it later adds (dpt_head.py:366-386).  w_packed = [3][3][Cin][Cout]. */
int32_t vgpa_conv3x3_f32(const float* x, const float* w_packed, const float* bias, const float* res, const float* res2, float* out,
                         int64_t N, int64_t H, int64_t W, int64_t Cin, int64_t Cout, int64_t stride, int32_t flags,
                         vgpa_stream_t stream);
/* 1x1 convolution on the same core: out [M,Cout] = x [M,Cin] . w_packed [Cin][Cout] + bias?  (projects.N, out_conv, and the
 * kernel = stride ConvTranspose2d as a GEMM in front of a pixel shuffle).  Every output element sums in the same order whatever M. */
int32_t vgpa_conv1x1_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t M, int64_t Cin, int64_t Cout,
                         vgpa_stream_t stream);
/* The end of DPTHead._forward_impl (dpt_head.py:229-247) in one launch: x [N,h,w,C] is sampled bilinearly (align_corners=True) at
 * the (H,W) grid, xtab [W,C/2] / ytab [H,C/2] (the 0.1-scaled halves of position_grid_to_embed; both NULL = no embedding) are
 * added, then 3x3 conv C -> 32 (w1_packed [3][3][C][32]) + b1 + ReLU, 1x1 conv 32 -> output_dim (w2 [output_dim][32]) + b2,
 * activate_head: preds [N,H,W,output_dim-1] (activation 0 exp, 1 inv_log), conf [N,H,W] = 1 + exp.  No [N,H,W,C] tensor is built. */
int32_t vgpa_dpt_tail_f32(const float* x, const float* xtab, const float* ytab, const float* w1_packed, const float* b1,
                          const float* w2, const float* b2, float* preds, float* conf, int64_t N, int64_t h, int64_t w, int64_t C,
                          int64_t H, int64_t W, int32_t output_dim, int32_t activation, vgpa_stream_t stream);
/* F.interpolate(bilinear, align_corners=True) of x [N,h,w,C] to out [N,H,W,C] (+ the separable embedding tables as above, or NULL). */
int32_t vgpa_upsample_bilinear_ac_f32(const float* x, const float* xtab, const float* ytab, float* out, int64_t N, int64_t h,
                                      int64_t w, int64_t C, int64_t H, int64_t W, vgpa_stream_t stream);
/* softmax(scale q k^T) v in fp32 for the camera trunk: S <= 128 tokens, D a multiple of 32 (<= 256), one workgroup per (batch, head).
 * q / k / v element (b,h,s,d) at base[b * stride_b + h * stride_h + s * stride_s + d]; o [B,S,H,D] contiguous. */
int32_t vgpa_attn_small_f32(const float* q, const float* k, const float* v, int64_t stride_b, int64_t stride_h, int64_t stride_s,
                            float* o, int64_t B, int64_t H, int64_t S, int64_t D, float scale, vgpa_stream_t stream);

/* ---- DINOv2 token embedding: DinoVisionTransformer.prepare_tokens_with_masks(x, masks=None), vggt/layers/vision_transformer.py:214-226
 * (PatchEmbed.forward, vggt/layers/patch_embed.py:63-78; interpolate_pos_encoding's RESULT is the `pos` argument) (csrc/dino_embed.hip) ----
 * images [N,3,H,W] NCHW contiguous, in_dtype 0 fp32 | 1 bf16, H and W multiples of `patch`; out [N, 1+R+P, C], P = (H/patch)(W/patch),
 * out_dtype 0 | 1:  row 0 = cls_token + pos[0];  rows 1..R = register_tokens (no position);  row 1+R+j = W . patch_j + bias + pos[1+j].
 * w_packed fp32 [k_packed][C] = the Conv2d weight [C,3,patch,patch] flattened to [C, 3 patch^2], transposed, zero-padded to k_packed =
 * 3 patch^2 rounded up to 16 rows; bias, cls_token [C], register_tokens [R][C] (NULL when R = 0), pos [1+P][C] fp32.  C a multiple of 32;
 * images, w_packed, pos and out 16-byte aligned.  One launch, an implicit GEMM on the exact-fp32 MFMA: every output element is one fp32
 * chain in k order, so results are bit-identical for any split of the N frames over calls. */
int32_t vgpa_dino_embed(const void* images, int32_t in_dtype, const float* w_packed, int64_t k_packed, const float* bias,
                        const float* cls_token, const float* register_tokens, const float* pos, void* out, int32_t out_dtype, int64_t N,
                        int64_t H, int64_t W, int64_t patch, int64_t C, int64_t R, vgpa_stream_t stream);
/* The DINOv2 residual stream in fp32 (vggt/layers/block.py:77-98 as bf16 autocast evaluates it; csrc/dino_stream.hip), forward only, rows [M][D]:
 * x_new = x + gamma * y (y bf16, gamma fp32 [D] = LayerScale; y, gamma and x_new all NULL skips the add), n = LayerNorm(x_new or x) * ln_w + ln_b in
 * n_dtype 0 fp32 | 1 bf16 (ln_w, ln_b and n all NULL skips the norm).  x_new must not alias x. */
int32_t vgpa_stream_ln_f32(const float* x, const void* y, const float* gamma, const float* ln_w, const float* ln_b, float* x_new, void* n,
                           int32_t n_dtype, int64_t M, int64_t D, float eps, vgpa_stream_t stream);

/* ---- LPIPS-VGG around the convolutions (lpips 0.1, lpips/lpips.py; csrc/lpips.hip): fp32, NHWC, forward only, 16-byte aligned bases ----
 * ScalingLayer + layout change in front of conv1_1: x [N,3,H,W] NCHW in [-1,1] -> out [N,H,W,16], channels 0..2 = (x - shift_c) / scale_c
 * (a true division), channels 3..15 = 0, so that conv1_1 runs on vgpa_conv3x3_f32 with a [3][3][16][64] weight whose rows 3..15 are zero.
 * flags bit0: x is in [0,1] and is mapped to 2 x - 1 first (upstream's normalize=True).  x is read one float at a time, so any float-aligned base
 * (a frame slice of a batch of odd-sized frames) is valid; out is 16-byte aligned. */
int32_t vgpa_lpips_input_f32(const float* x, float* out, int64_t N, int64_t H, int64_t W, float shift0, float shift1, float shift2,
                             float scale0, float scale1, float scale2, int32_t flags, vgpa_stream_t stream);
/* 2 x 2 max pool, stride 2, floor: x [N,H,W,C] -> out [N,H/2,W/2,C]; C a multiple of 4, H and W >= 2.  flags bit0: relu(x) is pooled. */
int32_t vgpa_maxpool2x2_f32(const float* x, float* out, int64_t N, int64_t H, int64_t W, int64_t C, int32_t flags, vgpa_stream_t stream);
/* One LPIPS layer: f0, f1 [N,H,W,C] (C a multiple of 4, <= 512), w [C] (the `lin` 1x1 convolution, no bias);
 *   value[n] = mean over the H W pixels of  sum_c w_c (f0_c / (||f0||_2 + 1e-10) - f1_c / (||f1||_2 + 1e-10))^2
 * (normalize_tensor, lin, spatial_average).  out fp32 [N] and / or total fp64 [N] (either may be NULL) receive it.
 * flags bit0: ReLU on both maps as they are loaded; bit1: total[n] += value instead of total[n] = value.
 * Fixed-order fp64 reduction, no float atomics: bit-identical from run to run, and a frame's value does not depend on N.
 * An all-zero pixel contributes exactly 0. */
size_t vgpa_lpips_layer_workspace_bytes(int64_t N, int64_t H, int64_t W, int64_t C);
int32_t vgpa_lpips_layer_f32(const float* f0, const float* f1, const float* w, float* out, double* total, int64_t N, int64_t H, int64_t W,
                             int64_t C, int32_t flags, void* workspace, size_t ws_bytes, vgpa_stream_t stream);

/* ---- Depth Anything 3's DINOv2 backbone between its blocks, and its camera decoding (csrc/da3.hip): fp32, forward only, 16-byte aligned bases ----
 * Tokens are x fp32 [B,S,N,C] (S views of N tokens, token 0 the class / camera token).  The reference view of a batch element lives in a DEVICE
 * int32 [B] buffer that the selection writes and the other entry points read; no entry point needs it on the host.
 *
 * select_reference_view, depth_anything_3/model/reference_view_selector.py:29-112, on token 0 of every view.  strategy 0 "first", 1 "middle" (S / 2),
 * 2 "saddle_balanced", 3 "saddle_sim_range"; S <= 64.  metrics fp64 [B,S,4] (may be NULL) receives per view: the mean off-diagonal cosine similarity,
 * the token's norm, the unbiased variance of the normalised token, and the score the strategy ranks by (the balance score sum |minmax(m) - 0.5|; for
 * strategy 3 the range of the view's similarity row).  Reductions run in fp64 in a fixed order; a tie resolves to the lowest index; S == 1 gives 0. */
int32_t vgpa_da3_ref_view(const float* x, int64_t B, int64_t S, int64_t N, int64_t C, int32_t strategy, double* metrics, int32_t* ref_idx,
                          vgpa_stream_t stream);
/* reorder_by_reference / restore_original_order, reference_view_selector.py:115-222, over whole [N][C] slabs: inverse == 0 writes
 * out[b, j] = in[b, order_j], order = [ref, 0, .., ref-1, ref+1, ..]; inverse != 0 undoes it.  A second tensor (b_in, b_out; both NULL for none) rides
 * in the same launch.  Never in place: an output that aliases an input is an invalid argument.  N * C a multiple of 4. */
int32_t vgpa_da3_view_gather(const float* a_in, float* a_out, const float* b_in, float* b_out, const int32_t* ref_idx, int32_t inverse, int64_t B,
                             int64_t S, int64_t N, int64_t C, vgpa_stream_t stream);
/* x[b, s, 0, :] = cam (vision_transformer.py:323-331), in place: per_view != 0 reads cam [B,S,C] (the caller's tokens), per_view == 0 reads the
 * camera_token parameter [2,C]: row 0 for view 0, row 1 for every other view.  No other row of x is touched. */
int32_t vgpa_da3_cam_token(float* x, const float* cam, int32_t per_view, int64_t B, int64_t S, int64_t N, int64_t C, vgpa_stream_t stream);
/* One out layer (vision_transformer.py:341-346,382-398 with cat_token) in one launch: feats [B,S,N-1,2C] = [local_x | LayerNorm(x) * ln_w + ln_b] of
 * tokens 1.., cam [B,S,2C] = [local_x | x] of token 0, un-normalised.  The local half and the camera row are bit-exact copies.  ref_idx != NULL
 * restores the original view order (output view t reads reordered position inverse_t); NULL reads views as they are.  C a multiple of 4;
 * feats may be NULL when N == 1. */
int32_t vgpa_da3_tap(const float* local_x, const float* x, const float* ln_w, const float* ln_b, float eps, const int32_t* ref_idx, float* feats,
                     float* cam, int64_t B, int64_t S, int64_t N, int64_t C, vgpa_stream_t stream);
/* DepthAnything3Net._process_camera_estimation, depth_anything_3/model/da3.py:209-221: pose_enc fp32 [n,9] (translation, scalar-last quaternion,
 * fov_h, fov_w; camera-to-world) -> ext fp32 [n,3,4] = its inverse [R^T | -R^T T] (world-to-camera), intr fp32 [n,3,3] with focal =
 * (size / 2) / max(tan(fov / 2), 1e-6) and the principal point at the image centre. */
int32_t vgpa_da3_pose_decode(const float* pose_enc, int64_t n, float image_h, float image_w, float* ext, float* intr, vgpa_stream_t stream);
/* The end of DualDPT's auxiliary branch (depth_anything_3/model/dualdpt.py:250-258) in one launch on the convolution core of vgpa_conv3x3_f32:
 * x [N,h,w,C] plus xtab [w,C/2] / ytab [h,C/2] (the 0.1-scaled halves of position_grid_to_embed at the map's own grid; both NULL = no embedding),
 * zero padding, 3x3 conv C -> 32 (w1_packed [3][3][C][32]) + b1, LayerNorm over the 32 channels of each pixel (ln_w, ln_b [32]; biased variance of
 * the centred values, rsqrt(var + eps)), ReLU, 1x1 conv 32 -> output_dim (w2 [output_dim][32]) + b2: preds [N,h,w,output_dim-1] as they are
 * (linear), conf [N,h,w] = 1 + exp.  The embedded tensor is never built.  C a multiple of 16, 2 <= output_dim <= 8. */
int32_t vgpa_dualdpt_aux_tail_f32(const float* x, const float* xtab, const float* ytab, const float* w1_packed, const float* b1,
                                  const float* ln_w, const float* ln_b, float eps, const float* w2, const float* b2, float* preds, float* conf,
                                  int64_t N, int64_t h, int64_t w, int64_t C, int32_t output_dim, vgpa_stream_t stream);
/* DepthAnything3Net._process_ray_pose_estimation (depth_anything_3/model/da3.py:181-201, utils/ray_utils.py:20-93,313-421; csrc/da3_ray_pose.hip): cameras
 * from the ray map by confidence-weighted RANSAC of a homography.  ray fp32 [V,N,6] with N = ph * pw, conf fp32 [V,N]; gx [pw] / gy [ph] are the plane
 * grid's coordinates (the source points, z = 1).  All arithmetic behind the fp32 inputs is fp64; no input is written; two calls on one input are
 * bit-identical.
 *   ray_weights  wm [V,N] = conf where |ray z| > z_threshold (strict, compared in fp32), else 0: the weights every later step and the caller's sort use.
 *   ray_ransac   cand int32 [V,n_sample]: point indices by descending wm; sample_idx int32 [n_iter,8]: positions in cand, one table for every view
 *                (an entry outside [0, n_sample) or a candidate outside [0, N) makes that hypothesis score 0).  Fits n_iter <= 128 homographies per
 *                view (smallest eigenvector of the 9 x 9 weighted DLT normal matrix, H / H[2,2]), scores each by the summed wm of the points whose
 *                reprojection error is < reproj_threshold (a non-finite error is an outlier) -> best int32 [V] (largest score, lowest index on a
 *                tie), inlier uint8 [V,N] of the winner, n_inliers int32 [V].  workspace: vgpa_da3_ray_pose_workspace_bytes(V, N, n_iter), 8-byte aligned.
 *   ray_refit    use uint8 [V,N] marks the points the refit reads -> H [V,3,3] (refitted, / H[2,2]), R [V,3,3], T [V,3] (mean of ray[3:] under wm over
 *                ALL points), focal [V,2] and pp [V,2] (normalised, image size 2), ext [V,3,4] = rows :3 of the inverse of [R|T], intr [V,3,3] in
 *                pixels of image_h x image_w, n_used int32 [V] = the number of marked points. */
size_t vgpa_da3_ray_pose_workspace_bytes(int64_t V, int64_t N, int64_t n_iter);
int32_t vgpa_da3_ray_weights(const float* ray, const float* conf, int64_t V, int64_t N, float z_threshold, float* wm, vgpa_stream_t stream);
int32_t vgpa_da3_ray_ransac(const float* ray, const float* wm, const float* gx, const float* gy, const int32_t* cand, const int32_t* sample_idx, int64_t V,
                            int64_t ph, int64_t pw, int64_t n_sample, int64_t n_iter, float z_threshold, double reproj_threshold, int32_t* best,
                            uint8_t* inlier, int32_t* n_inliers, void* workspace, size_t workspace_bytes, vgpa_stream_t stream);
int32_t vgpa_da3_ray_refit(const float* ray, const float* wm, const float* gx, const float* gy, const uint8_t* use, int64_t V, int64_t ph, int64_t pw,
                           float z_threshold, float image_h, float image_w, float* H, float* R, float* T, float* focal, float* pp, float* ext, float* intr,
                           int32_t* n_used, vgpa_stream_t stream);

/* ---- CogVideoX VAE encoder on one frame (diffusers' autoencoder_kl_cogvideox.py; videogpa_amd/vae.py, csrc/vae.hip): fp32, NHWC, forward only ----
 * The 3x3 convolution of vgpa_conv3x3_f32 with its zero padding given per side: pad_lo rows / columns in front of index 0, pad_hi behind the last
 * (each 0 | 1), Ho = (H + pad_lo + pad_hi - 3) / stride + 1.  CogVideoXDownsample3D is stride 2 with pad_lo = 0, pad_hi = 1.  out = conv(x) + bias? + res?.
 * The K sum (9 Cin products) runs in chains of 64 products that start from zero and are added up in order: the rounding error of one long fp32
 * chain grows with the square root of its length, and the encoder's outputs are held to 4 x the error of an fp32 CPU convolution.  So
 * pad_lo = pad_hi = 1 agrees with vgpa_conv3x3_f32 to rounding, not bit for bit; like it, every output sums in the same order whatever N, H, W. */
int32_t vgpa_conv3x3_pad_f32(const float* x, const float* w_packed, const float* bias, const float* res, float* out, int64_t N, int64_t H, int64_t W,
                             int64_t Cin, int64_t Cout, int64_t stride, int32_t pad_lo, int32_t pad_hi, vgpa_stream_t stream);
/* CogVideoXCausalConv3d over the frames of a chunk: x [N,T,H,W,Cin] -> out [N,T,H,W,Cout] = conv3x3x3(x) + bias? + res?, stride 1, spatial zero
 * padding 1, w_packed [3][3][3][Cin][Cout] (kt, ky, kx).  Temporal tap kt of output frame t reads frame t + kt - 2.  The two frames in front of
 * frame 0 are prev [N,2,H,W,Cin] (diffusers' conv_cache: the last two input frames of the chunk before); with prev NULL frame 0 stands in for
 * both (the first-frame replication).  Cin, Cout multiples of 16; x, prev and w_packed 16-byte aligned; never in place.  The K sum (27 Cin products,
 * tap-major) runs in the chains of 64 of vgpa_conv3x3_pad_f32.  CONTRACT: every output element sums the same products in the same order whatever
 * N and T are and whether its earlier frames come from prev or from x, so one call over T frames equals any split into two calls bit for bit when
 * the second gets the first's last two input frames as prev.  T = 1 without prev agrees with vgpa_conv3x3_pad_f32 on the tap-summed weight to
 * rounding only. */
int32_t vgpa_conv3x3x3_causal_f32(const float* x, const float* prev, const float* w_packed, const float* bias, const float* res, float* out, int64_t N,
                                  int64_t T, int64_t H, int64_t W, int64_t Cin, int64_t Cout, vgpa_stream_t stream);
/* CogVideoXDownsample3D in one launch: x [N,T,H,W,C] -> out [N,T',Ho,Wo,Cout], the stride-2 convolution of vgpa_conv3x3_pad_f32 with pad_lo = 0,
 * pad_hi = 1 (Ho = (H - 2) / 2 + 1; H, W >= 2) of the temporally pooled frames, which the loader forms and never writes.  compress_time 0: T' = T,
 * frame by frame.  compress_time 1: T' = (T + 1) / 2; output frame t' reads frames (2t', 2t' + 1) of an even T; of an odd T frame 0 alone for
 * t' = 0 and frames (2t' - 1, 2t') after it; a pooled value is (a + b) * 0.5 in fp32.  Bit for bit the result of pooling so on the host and
 * calling vgpa_conv3x3_pad_f32 on [N * T',H,W,C]. */
int32_t vgpa_vae_downsample_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t N, int64_t T, int64_t H, int64_t W,
                                int64_t C, int64_t Cout, int32_t compress_time, vgpa_stream_t stream);
/* Layout change in front of conv_in: x [N,3,H,W] NCHW contiguous (in_dtype 0 fp32 | 1 bf16) -> out fp32 [N,H,W,16], channels 3..15 = 0, so that the
 * stem runs on vgpa_conv3x3_f32 with a [3][3][16][Cout] weight whose rows 3..15 are zero.  out is 16-byte aligned. */
int32_t vgpa_vae_input_f32(const void* x, int32_t in_dtype, float* out, int64_t N, int64_t H, int64_t W, vgpa_stream_t stream);
/* GroupNorm statistics of x [N,HW,C] with G groups of C / G neighbouring channels: stats fp32 [N,G,2] = (mean, 1 / sqrt(biased variance + eps)).
 * C a multiple of 4 and of G, at most 1024.  Two stages, both deterministic: per workgroup and channel (mean, M2) by Welford's update, merged over
 * the workgroups and the group's channels with Chan's pairwise formula in a fixed order, all in fp64; no atomics and no sum of squares.  A
 * sample's statistics do not depend on N. */
size_t vgpa_groupnorm_stats_workspace_bytes(int64_t N, int64_t HW, int64_t C, int64_t G);
int32_t vgpa_groupnorm_stats_f32(const float* x, float* stats, int64_t N, int64_t HW, int64_t C, int64_t G, float eps, void* workspace,
                                 size_t ws_bytes, vgpa_stream_t stream);
/* out = silu((x - mean) * rstd * gamma + beta) with the statistics above; gamma, beta [C]; x, out, gamma and beta 16-byte aligned.  Never in place. */
int32_t vgpa_groupnorm_silu_f32(const float* x, const float* stats, const float* gamma, const float* beta, float* out, int64_t N, int64_t HW,
                                int64_t C, int64_t G, vgpa_stream_t stream);
/* DiagonalGaussianDistribution of moments fp32 [N,hw,2L] (mean | logvar on the channel axis): logvar is clamped to [-30, 20], std = exp(logvar / 2),
 * sample = (mean + std * noise) * scale.  Outputs are [N,L,hw] (= [N,L,1,h,w]) in out_dtype 0 fp32 | 1 bf16, rounded once from fp32; each of sample,
 * mean, logvar, std_out may be NULL (not all).  noise [N,L,hw] in out_dtype, or NULL for none (sample = mean * scale). */
int32_t vgpa_vae_sample(const float* moments, const void* noise, float scale, void* sample, void* mean, void* logvar, void* std_out,
                        int32_t out_dtype, int64_t N, int64_t hw, int64_t L, vgpa_stream_t stream);

/* ---- CogVideoX VAE decoder (videogpa_amd/vae.py with_decoder=True): the entry points above plus three ----
 * CogVideoXUpsample3D in one launch: x [N,T,H,W,C] -> out [N,T',2H,2W,Cout], the 3x3 padding-1 convolution of vgpa_conv3x3_pad_f32 (w_packed
 * [3][3][C][Cout], the K sum in its chains of 64) over the nearest-neighbour x2 map, which the loader forms by index arithmetic and never writes: tap
 * (y, x) of output frame t' reads source pixel (y >> 1, x >> 1) of source frame f(t'), zero outside [0,2H) x [0,2W).  compress_time 0, or T = 1:
 * T' = T, f(t') = t'.  compress_time 1 and an even T: T' = 2T, f(t') = t' >> 1.  compress_time 1 and an odd T > 1: T' = 2T - 1, f(0) = 0 and
 * f(t') = 1 + ((t' - 1) >> 1) (frame 0 is not doubled in time).  Bit for bit the result of up-sampling so on the host and calling
 * vgpa_conv3x3_pad_f32 on [N * T',2H,2W,C].  C, Cout multiples of 16; x and w_packed 16-byte aligned; never in place. */
int32_t vgpa_vae_upsample_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t N, int64_t T, int64_t H, int64_t W,
                              int64_t C, int64_t Cout, int32_t compress_time, vgpa_stream_t stream);
/* CogVideoXSpatialNorm3D followed by SiLU: out = silu(((x - mean) * rstd * gamma + beta) * Y + B) over x [N,T,H,W,C] with the statistics of
 * vgpa_groupnorm_stats_f32 (HW = T * H * W) and yb [N,t,h,w,2C] = (Y | B), conv_y | conv_b of the latent at the latent's resolution.  Pixel
 * (tt, y, x) reads yb at (tz(tt), y * h / H, x * w / W): the nearest-neighbour resize of the modulation maps, never formed.  tz(tt) =
 * floor(tt * t / T), except for an odd T > 1, where tz(0) = 0 and tz(tt) = 1 + floor((tt - 1) * (t - 1) / (T - 1)) (frame 0 of the latent goes
 * to frame 0 alone; needs t >= 2).  H a multiple of h, W of w, t <= T; everything 16-byte aligned; never in place. */
int32_t vgpa_spatial_norm_silu_f32(const float* x, const float* stats, const float* gamma, const float* beta, const float* yb, float* out, int64_t N,
                                   int64_t T, int64_t H, int64_t W, int64_t C, int64_t G, int64_t t, int64_t h, int64_t w, vgpa_stream_t stream);
/* Behind conv_out, run with its 3 output channels padded to 16: x fp32 [N,THW,16] -> out_dtype 0 fp32 | 1 bf16: out [N,3,THW], channels 0..2, rounded
 * once (the inverse of vgpa_vae_input_f32); out_dtype 2: out uint8 [N,THW,3] = round(clamp(x / 2 + 0.5, 0, 1) * 255), ties to even (the pipeline's
 * postprocess_video).  x is 16-byte aligned. */
int32_t vgpa_vae_output(const float* x, void* out, int32_t out_dtype, int64_t N, int64_t THW, vgpa_stream_t stream);

/* ---- T5 encoder between its GEMMs (transformers' T5EncoderModel, the CogVideoX text encoder; videogpa_amd/t5.py, csrc/t5.hip): forward only ----
 * o = softmax(q k^T + bias[h][j - i] + mask[b][j]) v at head_dim 64: T5 attention has no 1/sqrt(d) scale.  q, k, v are bf16 [B,H,S,64] views given
 * by element strides {batch, head, token} (slices of the fused QKV GEMM output, read in place; strides multiples of 8, bases 16-byte aligned);
 * o bf16 [B,S,H*64] contiguous.  1 <= S <= 512, anything else is an invalid argument.  bias_delta fp32 [H, 2S-1], indexed by j - i + S - 1 (key j,
 * query i): the relative-position bias as a per-head Toeplitz table.  mask uint8 [B,S], 1 = keep, or NULL for none: a masked key gets the weight
 * exactly 0, whatever k and v hold there; every sample must keep at least one key (its rows are NaN otherwise).  Padded query rows are computed like
 * any other.  bf16 MFMA for both products, fp32 scores / bias add / softmax, the exact two-pass softmax (true row maximum); the row sum adds the
 * bf16-rounded weights that multiply v.  A sample's result does not depend on B, and NULL equals an all-ones mask bit for bit. */
int32_t vgpa_t5_attn_fwd(const void* q, const void* k, const void* v, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                         const float* bias_delta, const uint8_t* mask, void* o, int64_t B, int64_t H, int64_t S, vgpa_stream_t stream);
/* The fp32 residual stream with T5LayerNorm (RMS only: no mean subtraction, no bias): x_new [M,D] fp32, then
 *   n = w * x_new * rsqrt(mean(x_new^2) + eps),  w fp32 [D],  stored in n_dtype 0 fp32 | 1 bf16, rounded once.
 * x_new is  x (y, ids NULL; x_new must be NULL),  x + y (y bf16 [M,D], the GEMM output in front; written to x_new unless that is NULL; never in place),
 * or the embedding row float(table[ids[row]]) (ids int64 [M], table bf16 [V,D]; x and y NULL, x_new required; an id outside [0,V) gives a row of NaN
 * and reads nothing).  D a multiple of 64, at most 4096. */
int32_t vgpa_t5_rms(const float* x, const void* y, const int64_t* ids, const void* table, int64_t V, const float* w, float* x_new, void* n,
                    int32_t n_dtype, int64_t M, int64_t D, float eps, vgpa_stream_t stream);
/* T5DenseGatedActDense between its GEMMs: u bf16 [M, 2 d_ff] (one GEMM against wi_0 | wi_1) -> g bf16 [M, d_ff] = gelu_new(u[:, :d_ff]) * u[:, d_ff:],
 * the tanh GELU and the product in fp32, rounded once.  d_ff a multiple of 8. */
int32_t vgpa_t5_gated_gelu(const void* u, void* g, int64_t M, int64_t d_ff, vgpa_stream_t stream);

/* ---- SuperPoint keypoint extractor (lightglue.SuperPoint; videogpa_amd/superpoint.py, csrc/superpoint.hip): fp32, channels-last, forward only ----
 * The 1x1 convolution of vgpa_conv1x1_f32 over relu(x): the producer stored its output before the ReLU.  Same kernel, same sums. */
int32_t vgpa_conv1x1_relu_f32(const float* x, const float* w_packed, const float* bias, float* out, int64_t M, int64_t Cin, int64_t Cout,
                              vgpa_stream_t stream);
/* Frames -> conv1a's output before its ReLU, out [T,Ho,Wo,64], in one launch.  mode 0: src uint8 [T,H,W,3] RGB, gray = (9798 R + 19235 G + 3735 B +
 * 16384) >> 15 (cv2's 8-bit RGB2GRAY restated from memory, not pinned), value = table[gray], table fp32 [256] made on the host as g / 255.0.
 * mode 1: src fp32 [T,1,H,W].  mode 3: src fp32 [T,3,H,W], value = 0.299 R + 0.587 G + 0.114 B.  table is NULL unless mode 0.  The value image is
 * resized to (Ho, Wo) as F.interpolate(mode="bilinear", align_corners=False) does in fp32: scale = in / out, src = max(scale (dst + 0.5) - 0.5, 0),
 * both lerps in torch's order; equal sizes copy exactly.  Then the 3x3 convolution 1 -> 64 with zero padding: w [3][3][1][64], bias [64], 16-byte
 * aligned like out.  gray, if not NULL, receives the resized value image [T,Ho,Wo]. */
int32_t vgpa_sp_input_conv1a(const void* src, int32_t mode, const float* table, const float* w, const float* bias, float* out, float* gray, int64_t T,
                             int64_t H, int64_t W, int64_t Ho, int64_t Wo, vgpa_stream_t stream);
/* Detector head: x [T,h,w,256] (convPa before its ReLU, 16-byte aligned) -> score [T,8h,8w]: relu, the 1x1 convolution w [256][65] + bias [65],
 * softmax over the 65, the last (dustbin) channel dropped, channel c of cell (cy, cx) to pixel (8 cy + c / 8, 8 cx + c % 8). */
int32_t vgpa_sp_head_f32(const float* x, const float* w, const float* bias, float* score, int64_t T, int64_t h, int64_t wd, vgpa_stream_t stream);
/* simple_nms of lightglue/superpoint.py on score [T,Hs,Ws] (finite values): mask = s == maxpool(s); twice { supp = maxpool(mask) > 0;
 * s' = where(supp, 0, s); mask |= (s' == maxpool(s')) & ~supp }; out = where(mask, s, 0), windows (2 radius + 1)^2 padded with -inf, radius 1..4.
 * Exact comparisons only: equal to torch bit for bit.  Then the outer `border` rows and columns are set to -1.  Never in place. */
int32_t vgpa_sp_nms_f32(const float* score, float* out, int64_t T, int64_t Hs, int64_t Ws, int32_t radius, int32_t border, vgpa_stream_t stream);
/* Keypoints of nms [T,Hs,Ws]: the pixels with nms > threshold.  A frame with at most kcap of them keeps all, in row-major order; a frame with more
 * keeps the kcap highest, in descending score, equal scores in row-major order (at the cut too).  kp fp32 [T,kcap,2] = (x, y), sc fp32 [T,kcap],
 * counts int32 [T]; rows past a frame's count are not written.  kcap <= 4096 or kcap >= Hs Ws.  Deterministic.  workspace 256-byte aligned. */
size_t vgpa_sp_select_workspace_bytes(int64_t T, int64_t Hs, int64_t Ws);
int32_t vgpa_sp_select(const float* nms, float threshold, int64_t T, int64_t Hs, int64_t Ws, int64_t kcap, float* kp, float* sc, int32_t* counts,
                       void* workspace, size_t ws_bytes, vgpa_stream_t stream);
/* sample_descriptors with s = 8 on the raw descriptor map dmap [T,h,w,256] (convDb's output, 16-byte aligned): out [T,kcap,256] row i of frame t =
 * normalize(bilinear(normalize(dmap))) at kp [T,kcap,2], for i < counts[t]; normalize is x / max(|x|_2, 1e-12), the sample grid_sample's
 * (align_corners=True, zeros outside) at ((kp - 3.5) / (8 w - 4.5), (.. h ..)) mapped to [-1, 1]. */
int32_t vgpa_sp_sample_desc_f32(const float* dmap, const float* kp, const int32_t* counts, float* out, int64_t T, int64_t h, int64_t wd, int64_t kcap,
                                vgpa_stream_t stream);

/* ---- LightGlue (features = "superpoint": 256 features, 4 heads of 64) between its GEMMs: csrc/lightglue.hip.  Forward only, fp32 in and out.
 * Variable-length form: a sample owns R rows of an activation; rows [0, S0) are image 0 with count c0[b], rows [S0, R) image 1 with count c1[b]
 * (c1 NULL: one segment and S0 == R).  Counts are device int32 [B], clamped to the segment; rows at or past a count are never read as keys and never
 * written.  A sample's result does not depend on B, on R or on the other samples, bit for bit; no float atomics; at most 4096 rows per segment. */
/* The Linears and sim in exact fp32 (v_mfma_f32_32x32x2_f32): c[b c_batch_stride + r ldc + n] = alpha sum_k a[b a_batch_stride + r lda + k]
 * bm[b b_batch_stride + n ldb + k] + bias[n] for r < R, n < N, or, with accumulate (then bias is NULL), c += alpha sum.  Both operands are row-major
 * over k: bm is an nn.Linear weight [N][K] as it stands (batch stride 0) or a second activation.  K is a multiple of 16; a, bm 16-byte aligned, lda, ldb
 * and their batch strides multiples of 4.  Every element is one fixed sum over k that does not depend on B, R, N or the element's place: a row's result is
 * the same bits in any batch.  c0 not NULL: only rows below the counts of the segments (S0, c0, c1) are computed and written; cn (int32 [B], may be
 * NULL): only columns below cn[b]. */
int32_t vgpa_lg_gemm(const float* a, int64_t a_batch_stride, int64_t lda, const float* bm, int64_t b_batch_stride, int64_t ldb, const float* bias, float* c,
                     int64_t c_batch_stride, int64_t ldc, int64_t B, int64_t R, int64_t N, int64_t K, float alpha, int32_t accumulate, int64_t S0,
                     const int32_t* c0, const int32_t* c1, const int32_t* cn, vgpa_stream_t stream);
/* o = softmax(q k^T / 8) v per head of 64.  ptrs holds, per direction, {q, k, v, o, nq, nk, qcos, qsin, kcos, ksin} (10 pointers) and strides
 * {q_b, q_h, q_t, k_b, k_h, k_t, v_b, v_h, v_t, o_b, o_t, rq_b, rk_b, nq_max, nk_max, 0} (16 values, in elements): q, k, v are fp32 views whose element
 * (b, h, t, d) is at b x_b + h x_h + t x_t + d dim_stride, dim_stride 1 or 3 (3: the interleaved Wqkv output read in place); o fp32 with head h at
 * o[b o_b + t o_t + 64 h], 16-byte aligned rows; nq / nk int32 [B]; the rotary tables fp32 [.][32] cos and sin with batch stride rq_b / rk_b, or NULL.
 * The loader forms rope(x) q_premul in fp32 for q and k and rounds once to fp16; both products are fp16 MFMA with fp32 accumulators, the softmax is fp32
 * and online, the weights are rounded to fp16 and normalised by their rounded sum.  nk = 0: the nq rows are written as 0.  ndir 1 or 2 directions
 * (blockIdx.z) in one launch. */
int32_t vgpa_lg_attn_fwd(const void* const* ptrs, const int64_t* strides, int64_t B, int64_t H, int64_t ndir, int64_t dim_stride, float q_premul,
                         vgpa_stream_t stream);
/* cos / sin of p = Wr k' (Wr fp32 [32][2]) for kpts [B,N,2], k' = (k - size / 2) / (max(size) / 2), size = image_size [B,2] or, when NULL,
 * 1 + max - min over the sample's own keypoints; row i of sample b goes to out[b out_batch_stride + 32 i ..]. */
int32_t vgpa_lg_posenc(const float* kpts, const int32_t* counts, const float* image_size, const float* Wr, float* cos_out, float* sin_out, int64_t B, int64_t N,
                       int64_t out_batch_stride, vgpa_stream_t stream);
/* h [B R][512] = gelu_erf(LayerNorm(u [B R][512]; gamma, beta, eps)).  resid not NULL: resid[row resid_stride + 0..255] += resid_bias, the bias of the
 * GEMM that then accumulates into the residual stream. */
int32_t vgpa_lg_ln_gelu(const float* u, const float* gamma, const float* beta, float eps, float* h, float* resid, int64_t resid_stride, const float* resid_bias,
                        int64_t B, int64_t R, int64_t S0, const int32_t* c0, const int32_t* c1, vgpa_stream_t stream);
/* z = w . x[row] + bias over 256 features, conf = sigmoid(z) (either output may be NULL); below[b] += number of the sample's rows with conf < thr,
 * compared in double (below is zeroed by the caller; an integer count). */
int32_t vgpa_lg_confidence(const float* x, int64_t x_stride, const float* w, float bias, float* conf, float* z, double thr, int32_t* below, int64_t B, int64_t R,
                           int64_t S0, const int32_t* c0, const int32_t* c1, vgpa_stream_t stream);
/* Point pruning.  A segment with more than prune_min rows keeps row i iff match[i] > thr_keep or conf[i] <= thr_conf (in double); any other keeps all and
 * leaves prune alone.  Kept rows move, in order, to the front of the segment of the OUTPUT buffers (never in place): 256 features of x, the rotary
 * tables [B R][32], ind; prune{0,1}[b][ind] += 1 ([B][P0], [B][P1]); c{0,1}_out = rows kept; keep_out (may be NULL) the mask by input row. */
int32_t vgpa_lg_prune(const float* conf, const float* match, double thr_conf, double thr_keep, int64_t prune_min, const float* x_in, float* x_out, int64_t x_stride,
                      const float* cos_in, const float* sin_in, float* cos_out, float* sin_out, const int32_t* ind_in, int32_t* ind_out, int32_t* prune0,
                      int32_t* prune1, int64_t P0, int64_t P1, int64_t B, int64_t R, int64_t S0, const int32_t* c0, const int32_t* c1, int32_t* c0_out,
                      int32_t* c1_out, uint8_t* keep_out, vgpa_stream_t stream);
/* Assignment from sim [B,Mmax,Nmax], the matchability logits z0 [B,Mmax], z1 [B,Nmax] and the counts m, n.  stages is a bit set:
 * 1 = max and log-sum-exp of sim by row and column; 2 = maximum and argmax by row and column of the log score
 * ((sim - rmax) - rlog) + ((sim - cmax) - clog) + (logsigmoid(z0) + logsigmoid(z1)), TIES TO THE LOWEST INDEX as torch.max on the CPU, and, if scores is
 * not NULL, the full log assignment with its dustbins in scores [B,Mmax+1,Nmax+1] (dustbin row at m, column at n); 4 = mutual check, exp, score > thr
 * (double): matches0 [B,M0] / matches1 [B,N0] / mscores0 / mscores1 (pre-filled by the caller with -1 / 0; written through ind0 / ind1 [B,Mmax] / [B,Nmax]
 * when given) and the valid (i, j) in row order in matches [B,M0,2] with mscores [B,M0] and nmatch [B].  The workspace holds, as fp32 / int32 words,
 * rmax, rlog, rbest, rarg [B Mmax] each, then cmax, clog, cbest, carg [B Nmax] each. */
size_t vgpa_lg_assign_workspace_bytes(int64_t B, int64_t Mmax, int64_t Nmax);
int32_t vgpa_lg_assign(const float* sim, const float* z0, const float* z1, const int32_t* m, const int32_t* n, int64_t B, int64_t Mmax, int64_t Nmax, double thr,
                       const int32_t* ind0, const int32_t* ind1, int64_t M0, int64_t N0, int32_t* matches0, int32_t* matches1, float* mscores0, float* mscores1,
                       int32_t* matches, float* mscores, int32_t* nmatch, float* scores, int32_t stages, void* workspace, size_t ws_bytes, vgpa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VIDEOGPA_HIP_H */
