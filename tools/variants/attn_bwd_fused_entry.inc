// variant builds only (tools/build_variant.sh, -DVGPA_VARIANTS): #included by videogpa_amd/csrc/attention.hip at the place this code used to stand.
// 
// fused backward: dK, dV (bf16 views) and dQ accumulated into dq_f32 -- fp32 [B,H,S,64] contiguous, ZEROED BY THE CALLER.
int32_t vgpa_attn_bwd_fused(const void* q, const void* k, const void* v, const void* d_o, const float* lse2, const float* delta,
                            float* dq_f32, void* dk, void* dv, const int64_t* q_strides, const int64_t* k_strides,
                            const int64_t* v_strides, const int64_t* do_strides, const int64_t* dk_strides, const int64_t* dv_strides,
                            int64_t B, int64_t H, int64_t S, int64_t head_dim, float scale, hipStream_t stream) {
    if (!q || !k || !v || !d_o || !lse2 || !delta || !dq_f32 || !dk || !dv || !bwd_common_ok(B, H, S, head_dim)) return VGPA_ERR_INVALID;
    if (!view_ok(q_strides, B, H, S, HD) || !view_ok(k_strides, B, H, S, HD) || !view_ok(v_strides, B, H, S, HD) || !view_ok(do_strides, B, H, S, HD) ||
        !view_ok(dk_strides, B, H, S, HD) || !view_ok(dv_strides, B, H, S, HD) || !al16(q) || !al16(k) || !al16(v) || !al16(d_o) || !al16(dk) || !al16(dv))
        return VGPA_ERR_INVALID;
    const int n_t = (int)((S + FUSED_KEYS - 1) / FUSED_KEYS);
    VGPA_LAUNCH(attn_bwd_fused_kernel, dim3((unsigned)((int64_t)n_t * B * H)), dim3(512), 0, stream, (const bf16_t*)q, (const bf16_t*)k,
                (const bf16_t*)v, (const bf16_t*)d_o, lse2, delta, dq_f32, (bf16_t*)dk, (bf16_t*)dv, mk(q_strides), mk(k_strides),
                mk(v_strides), mk(do_strides), mk(dk_strides), mk(dv_strides), (int)S, (int)H, n_t, scale, 0.6931471805599453f);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

