// LayerNorm pieces shared by the one-wave-per-row kernels (csrc/norm.hip, csrc/residual_ln.hip, csrc/wan.hip): a row of D <= 4096 elements is held by a
// wave as v[NV][8], chunk c of lane l covering elements (c * 64 + l) * 8 .. + 7.
#pragma once
#include "common.h"

// second pass of the exact two-pass variance over eight elements of the row: sq += (v - mean)^2, in element order
__device__ __forceinline__ void ln_sqdev_acc8(const float* v, float mean, float& sq) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float d = v[j] - mean; sq += d * d; }
}

// LayerNorm backward of one element: g = the incoming gradient times the affine, c1 = mean(g), c2 = mean(g * xhat) over the row
__device__ __forceinline__ float ln_bwd_dx(float rstd, float g, float xhat, float c1, float c2) { return rstd * (g - c1 - xhat * c2); }

// CALL with `constexpr int NV` = the number of 512-element chunks of a D-wide row
#define ROW_DISPATCH_NV(D, CALL)                       \
    switch (((D) + 511) / 512) {                       \
        case 1: { constexpr int NV = 1; CALL; } break; \
        case 2: { constexpr int NV = 2; CALL; } break; \
        case 3: { constexpr int NV = 3; CALL; } break; \
        case 4: { constexpr int NV = 4; CALL; } break; \
        case 5: { constexpr int NV = 5; CALL; } break; \
        case 6: { constexpr int NV = 6; CALL; } break; \
        case 7: { constexpr int NV = 7; CALL; } break; \
        case 8: { constexpr int NV = 8; CALL; } break; \
        default: return VGPA_ERR_INVALID;              \
    }
