// Depth Anything 3 input processing on the device: depth_anything_3/utils/io/input_processor.py (cv2.resize INTER_AREA / INTER_CUBIC of 8-bit RGB frames,
// centre crop, ToTensor + Normalize) and api.py:_add_processed_images, i.e. everything between the caller's uint8 frames and the network's input.
//   frames uint8 [T, H, W, 3]  ->  uint8 [T, out_h, out_w, 3]                                   (a resize that another stage follows)
//                              ->  x fp32 [T, 3, h, w] + processed_images uint8 [T, h, w, 3]    (the last stage: a resize's epilogue, or the kernel of
//                                                                                                 its own behind a crop / for frames that need no resize)
// The sizes, the choice of mode per stage and the crop boxes are host arithmetic in Python (videogpa_amd/da3_input.py:plan).
//
// PARITY WITH cv2 IS RESTATED, NOT PINNED.  OpenCV is not a dependency of this project and its own 8-bit result varies by build (a float SIMD vertical
// pass, IPP, half-up against half-even on the 2 x 2 path), so no OpenCV build is claimed bit for bit; tests/test_gpu_da3_input.py bounds these kernels
// against what the operations mean (float64 oracles in tests/da3_input_ref.py), as generate.py does for diffusers.  What is restated:
//
// AREA (INTER_AREA, out <= in on both axes; anything else is refused: the reference only picks area when not upscaling).  scale = 1.0 / ((double)out / in).
//   general path: the tap table of computeResizeAreaTab per output sample dx --
//       f1 = dx scale, f2 = f1 + scale, cell = min(scale, in - f1), s1 = ceil(f1), s2 = min(floor(f2), in - 1), s1 = min(s1, s2);
//       a left tap (s1 - 1, (s1 - f1) / cell) only if s1 - f1 > 1e-3, full taps 1 / cell on [s1, s2), a right tap (s2, min(min(f2 - s2, 1), cell) / cell) only if
//       f2 - s2 > 1e-3 -- made in double (da3_area_tab_kernel), each weight rounded to fp32; fp32 accumulation in ResizeArea_'s order: the row sum over the
//       x taps first, then sum += beta * row over the y taps; round-half-even with saturation.  Contraction is off: every product is rounded before its add.
//   CHOICE 1, both scales integer (|scale - (int)scale| < DBL_EPSILON on both axes): the integer box sum.  2 x 2 is (sum + 2) >> 2, which is what OpenCV's
//       vector path computes and what every row but its last few columns gets (its scalar tail rounds half-even instead); any other integer scale is the
//       round-half-even of sum * (1.f / area), as ResizeAreaFast_ computes it.
//   CHOICE 2: one integer axis does not make the fast path; it takes the general one (as in OpenCV).
//
// CUBIC (INTER_CUBIC, any size), integer work end to end like the PIL kernels of preprocess.hip:
//   fx = (float)((dx + 0.5) scale - 0.5), sx = floor(fx), fx -= sx; four taps at sx - 1 .. sx + 2 with indices clamped to the image; Keys weights with A = -0.75
//   in fp32 (interpolateCubic), each fixed to short(rint(c 2048)) with no re-normalisation; the horizontal pass keeps int32 unshifted, the vertical pass is
//   (acc + (1 << 21)) >> 22, saturated.  |acc| <= 255 (2048 x 1.375)^2 + 2^21 < 2^31 (1.375 = the largest sum of |weights|, at fx = 0.5).
//
// LAST STAGE: x = (u / 255 - mean) / std, each step rounded in fp32 (ToTensor's div, Normalize's sub_ then div_; IEEE division); processed_images = table[c][u], a
//   3 x 256 byte table the host makes with api.py's expression (it is not always u).  One read of the source, one write of each output, no fp32 image in between.
#include "common.h"
#include <float.h>

#define DA3_AREA 0
#define DA3_CUBIC 1
#define DA3_CUBIC_BITS 11

static inline size_t di_al(size_t x) { return (x + 255) & ~(size_t)255; }
static inline double di_scale(int in, int out) { return 1.0 / ((double)out / (double)in); }
static inline int di_area_ks(int in, int out) { return (int)ceil(di_scale(in, out)) + 2; }      // left + ceil(scale) full + right
static inline bool di_int_scale(int in, int out, int* is) {
    const double s = di_scale(in, out);
    *is = (int)s;
    return fabs(s - (double)*is) < DBL_EPSILON && (int64_t)out * *is == in;
}

// ---- tables: one thread per output sample of one axis -----------------------------------------------------------------------------------------------------
// area: bounds[dx] = {first source sample, tap count}, w[dx][0 .. ks)
__global__ __launch_bounds__(64) void da3_area_tab_kernel(int in_size, int out_size, int ks, int* __restrict__ bounds, float* __restrict__ w) {
#pragma clang fp contract(off)
    const int dx = blockIdx.x * 64 + threadIdx.x;
    if (dx >= out_size) return;
    const double scale = 1.0 / ((double)out_size / (double)in_size);
    const double f1 = dx * scale, f2 = f1 + scale;
    const double cell = fmin(scale, in_size - f1);
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    s2 = s2 < in_size - 1 ? s2 : in_size - 1;
    s1 = s1 < s2 ? s1 : s2;
    float* k = w + (size_t)dx * ks;
    int n = 0, first = s1;
    if (s1 - f1 > 1e-3) {
        first = s1 - 1;
        k[n++] = (float)((s1 - f1) / cell);
    }
    for (int s = s1; s < s2 && n < ks; ++s) k[n++] = (float)(1.0 / cell);
    if (f2 - s2 > 1e-3 && n < ks) k[n++] = (float)(fmin(fmin(f2 - s2, 1.0), cell) / cell);
    if (first < 0) first = 0;
    if (first + n > in_size) n = in_size - first;      // cannot happen (s2 <= in - 1); keeps every read inside the image whatever the arguments
    bounds[2 * dx] = first;
    bounds[2 * dx + 1] = n;
}

// cubic: tab[dx] = {sx, c0, c1, c2, c3} (the weights as the shorts they are fixed to)
__global__ __launch_bounds__(64) void da3_cubic_tab_kernel(int in_size, int out_size, int* __restrict__ tab) {
#pragma clang fp contract(off)
    const int dx = blockIdx.x * 64 + threadIdx.x;
    if (dx >= out_size) return;
    const double scale = 1.0 / ((double)out_size / (double)in_size);
    float fx = (float)((dx + 0.5) * scale - 0.5);
    const int sx = (int)floorf(fx);
    fx -= (float)sx;
    const float A = -0.75f;
    float c[4];
    c[0] = ((A * (fx + 1.f) - 5.f * A) * (fx + 1.f) + 8.f * A) * (fx + 1.f) - 4.f * A;
    c[1] = ((A + 2.f) * fx - (A + 3.f)) * fx * fx + 1.f;
    c[2] = ((A + 2.f) * (1.f - fx) - (A + 3.f)) * (1.f - fx) * (1.f - fx) + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
    int* t = tab + (size_t)dx * 5;
    t[0] = sx;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float q = rintf(c[i] * (float)(1 << DA3_CUBIC_BITS));
        t[1 + i] = (int)(short)fminf(fmaxf(q, -32768.f), 32767.f);
    }
}

// ---- where a pixel of the last stage goes ---------------------------------------------------------------------------------------------------------------
struct Da3Out {
    uint8_t* u8;            // [T, out_h, out_w, 3], or
    float* x;               // [T, 3, out_h, out_w] with
    uint8_t* processed;     // [T, out_h, out_w, 3] = table[c][u]
    const uint8_t* table;   // [3][256]
};

__device__ __forceinline__ float da3_normalize(int u, int c) {
#pragma clang fp contract(off)
    const float mean = c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f);
    const float sd = c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f);
    const float v = (float)u / 255.0f;
    return (v - mean) / sd;
}

template <bool NORM>
__device__ __forceinline__ void da3_store(const Da3Out& o, int t, int y, int x, int out_h, int out_w, const int* v) {
    const size_t plane = (size_t)out_h * out_w;
    const size_t pix = ((size_t)t * out_h + y) * out_w + x;
    if (NORM) {
        float* xo = o.x + (size_t)t * 3 * plane + (size_t)y * out_w + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            xo[c * plane] = da3_normalize(v[c], c);
            o.processed[pix * 3 + c] = o.table[c * 256 + v[c]];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o.u8[pix * 3 + c] = (uint8_t)v[c];
    }
}

__device__ __forceinline__ int da3_sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---- area, general path: one thread per output pixel, blockIdx.y = output row (its y taps are uniform over the block) --------------------------------------
template <bool NORM>
__global__ __launch_bounds__(256) void da3_area_kernel(const uint8_t* __restrict__ src, int H, int W, int out_h, int out_w, int ks_x, int ks_y,
                                                         const int* __restrict__ bx, const float* __restrict__ wx, const int* __restrict__ by,
                                                         const float* __restrict__ wy, Da3Out o) {
#pragma clang fp contract(off)
    const int dx = blockIdx.x * 256 + threadIdx.x;
    if (dx >= out_w) return;
    const int dy = blockIdx.y, t = blockIdx.z;
    const int x0 = bx[2 * dx], nx = bx[2 * dx + 1], y0 = by[2 * dy], ny = by[2 * dy + 1];
    const float* kx = wx + (size_t)dx * ks_x;
    const float* ky = wy + (size_t)dy * ks_y;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < ny; ++j) {
        const uint8_t* row = src + (((size_t)t * H + y0 + j) * W + x0) * 3;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        for (int i = 0; i < nx; ++i) {
            const float a = kx[i];
            r0 += (float)row[3 * i] * a; r1 += (float)row[3 * i + 1] * a; r2 += (float)row[3 * i + 2] * a;
        }
        const float b = ky[j];
        s0 += b * r0; s1 += b * r1; s2 += b * r2;
    }
    const int v[3] = {da3_sat8((int)rintf(s0)), da3_sat8((int)rintf(s1)), da3_sat8((int)rintf(s2))};
    da3_store<NORM>(o, t, dy, dx, out_h, out_w, v);
}

// ---- area, both scales integer: the box sum ------------------------------------------------------------------------------------------------------------------
template <bool NORM>
__global__ __launch_bounds__(256) void da3_area_int_kernel(const uint8_t* __restrict__ src, int H, int W, int out_h, int out_w, int isx, int isy, Da3Out o) {
#pragma clang fp contract(off)
    const int dx = blockIdx.x * 256 + threadIdx.x;
    if (dx >= out_w) return;
    const int dy = blockIdx.y, t = blockIdx.z;
    int a0 = 0, a1 = 0, a2 = 0;
    for (int j = 0; j < isy; ++j) {
        const uint8_t* row = src + (((size_t)t * H + (size_t)dy * isy + j) * W + (size_t)dx * isx) * 3;
        for (int i = 0; i < isx; ++i) { a0 += row[3 * i]; a1 += row[3 * i + 1]; a2 += row[3 * i + 2]; }
    }
    int v[3];
    if (isx == 2 && isy == 2) {
        v[0] = (a0 + 2) >> 2; v[1] = (a1 + 2) >> 2; v[2] = (a2 + 2) >> 2;
    } else {
        const float inv = 1.f / (float)(isx * isy);
        v[0] = da3_sat8((int)rintf((float)a0 * inv)); v[1] = da3_sat8((int)rintf((float)a1 * inv)); v[2] = da3_sat8((int)rintf((float)a2 * inv));
    }
    da3_store<NORM>(o, t, dy, dx, out_h, out_w, v);
}

// ---- cubic: one thread per output pixel, 4 x 4 taps, int32 ---------------------------------------------------------------------------------------------------
template <bool NORM>
__global__ __launch_bounds__(256) void da3_cubic_kernel(const uint8_t* __restrict__ src, int H, int W, int out_h, int out_w, const int* __restrict__ tx,
                                                          const int* __restrict__ ty, Da3Out o) {
    const int dx = blockIdx.x * 256 + threadIdx.x;
    if (dx >= out_w) return;
    const int dy = blockIdx.y, t = blockIdx.z;
    const int* cx = tx + (size_t)dx * 5;
    const int* cy = ty + (size_t)dy * 5;
    const int sx = cx[0], sy = cy[0];
    int xi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int x = sx - 1 + i;
        xi[i] = (x < 0 ? 0 : (x > W - 1 ? W - 1 : x)) * 3;
    }
    int a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int y = sy - 1 + j;
        y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
        const uint8_t* row = src + ((size_t)t * H + y) * (size_t)W * 3;
        int r0 = 0, r1 = 0, r2 = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int a = cx[1 + i];
            r0 += (int)row[xi[i]] * a; r1 += (int)row[xi[i] + 1] * a; r2 += (int)row[xi[i] + 2] * a;
        }
        const int b = cy[1 + j];
        a0 += r0 * b; a1 += r1 * b; a2 += r2 * b;
    }
    const int sh = 2 * DA3_CUBIC_BITS, half = 1 << (sh - 1);
    const int v[3] = {da3_sat8((a0 + half) >> sh), da3_sat8((a1 + half) >> sh), da3_sat8((a2 + half) >> sh)};
    da3_store<NORM>(o, t, dy, dx, out_h, out_w, v);
}

// ---- the last stage alone: crop box (top, left, h, w) of uint8 [T, H, W, 3] -> x, processed_images ------------------------------------------------------------
__global__ __launch_bounds__(256) void da3_normalize_kernel(const uint8_t* __restrict__ src, int H, int W, int top, int left, int h, int w, Da3Out o) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const int y = blockIdx.y, t = blockIdx.z;
    const uint8_t* px = src + (((size_t)t * H + top + y) * W + left + x) * 3;
    const int v[3] = {px[0], px[1], px[2]};
    da3_store<true>(o, t, y, x, h, w, v);
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------------------
static bool di_sizes_ok(int T, int H, int W, int out_h, int out_w, int mode) {
    if (T <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || (mode != DA3_AREA && mode != DA3_CUBIC)) return false;
    if (T > 65535 || out_h > 65535 || H > (1 << 20) || W > (1 << 20) || out_w > (1 << 20)) return false;
    if (mode == DA3_AREA && (out_h > H || out_w > W)) return false;
    return true;
}

extern "C" size_t vgpa_da3_resize_workspace_bytes(int32_t H, int32_t W, int32_t out_h, int32_t out_w, int32_t mode) {
    if (!di_sizes_ok(1, H, W, out_h, out_w, mode)) return 0;
    if (mode == DA3_CUBIC) return di_al((size_t)out_w * 5 * 4) + di_al((size_t)out_h * 5 * 4);
    int isx, isy;
    if (di_int_scale(W, out_w, &isx) && di_int_scale(H, out_h, &isy)) return 0;
    return di_al((size_t)out_w * (2 + di_area_ks(W, out_w)) * 4) + di_al((size_t)out_h * (2 + di_area_ks(H, out_h)) * 4);
}

#define DA3_LAUNCH_EPI(kernel, ...)                                                   \
    do {                                                                              \
        if (norm) VGPA_LAUNCH((kernel<true>), grid, dim3(256), 0, stream, __VA_ARGS__); \
        else VGPA_LAUNCH((kernel<false>), grid, dim3(256), 0, stream, __VA_ARGS__);     \
    } while (0)

extern "C" int32_t vgpa_da3_resize(const void* frames, int32_t T, int32_t H, int32_t W, int32_t out_h, int32_t out_w, int32_t mode, void* out_u8, float* x,
                                   void* processed, const void* table, void* workspace, size_t ws_bytes, hipStream_t stream) {
    if (!frames || !di_sizes_ok(T, H, W, out_h, out_w, mode)) return VGPA_ERR_INVALID;
    const bool norm = out_u8 == nullptr;
    if (norm ? (!x || !processed || !table) : (x || processed || table)) return VGPA_ERR_INVALID;   // one destination: the uint8 image, or the last stage's pair
    const size_t need = vgpa_da3_resize_workspace_bytes(H, W, out_h, out_w, mode);
    if (need && (!workspace || ws_bytes < need)) return VGPA_ERR_WORKSPACE;
    const Da3Out o = {(uint8_t*)out_u8, x, (uint8_t*)processed, (const uint8_t*)table};
    const uint8_t* src = (const uint8_t*)frames;
    const dim3 grid((out_w + 255) / 256, out_h, T);
    uint8_t* ws = (uint8_t*)workspace;
    if (mode == DA3_CUBIC) {
        int* tx = (int*)ws;
        int* ty = (int*)(ws + di_al((size_t)out_w * 5 * 4));
        VGPA_LAUNCH(da3_cubic_tab_kernel, dim3((out_w + 63) / 64), dim3(64), 0, stream, W, out_w, tx);
        VGPA_LAUNCH(da3_cubic_tab_kernel, dim3((out_h + 63) / 64), dim3(64), 0, stream, H, out_h, ty);
        DA3_LAUNCH_EPI(da3_cubic_kernel, src, H, W, out_h, out_w, tx, ty, o);
        VGPA_CHECK_LAUNCH();
        return VGPA_OK;
    }
    int isx, isy;
    if (di_int_scale(W, out_w, &isx) && di_int_scale(H, out_h, &isy)) {
        DA3_LAUNCH_EPI(da3_area_int_kernel, src, H, W, out_h, out_w, isx, isy, o);
        VGPA_CHECK_LAUNCH();
        return VGPA_OK;
    }
    const int ks_x = di_area_ks(W, out_w), ks_y = di_area_ks(H, out_h);
    int* bx = (int*)ws;
    float* wx = (float*)(bx + 2 * (size_t)out_w);
    ws += di_al((size_t)out_w * (2 + ks_x) * 4);
    int* by = (int*)ws;
    float* wy = (float*)(by + 2 * (size_t)out_h);
    VGPA_LAUNCH(da3_area_tab_kernel, dim3((out_w + 63) / 64), dim3(64), 0, stream, W, out_w, ks_x, bx, wx);
    VGPA_LAUNCH(da3_area_tab_kernel, dim3((out_h + 63) / 64), dim3(64), 0, stream, H, out_h, ks_y, by, wy);
    DA3_LAUNCH_EPI(da3_area_kernel, src, H, W, out_h, out_w, ks_x, ks_y, bx, wx, by, wy, o);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

extern "C" int32_t vgpa_da3_normalize(const void* image_u8, int32_t T, int32_t H, int32_t W, int32_t top, int32_t left, int32_t h, int32_t w, float* x,
                                      void* processed, const void* table, hipStream_t stream) {
    if (!image_u8 || !x || !processed || !table || T <= 0 || T > 65535 || H <= 0 || W <= 0 || h <= 0 || w <= 0 || h > 65535) return VGPA_ERR_INVALID;
    if (top < 0 || left < 0 || (int64_t)top + h > H || (int64_t)left + w > W) return VGPA_ERR_INVALID;
    const Da3Out o = {nullptr, x, (uint8_t*)processed, (const uint8_t*)table};
    VGPA_LAUNCH(da3_normalize_kernel, dim3((w + 255) / 256, h, T), dim3(256), 0, stream, (const uint8_t*)image_u8, H, W, top, left, h, w, o);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}
