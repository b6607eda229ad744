// Depth Anything 3's ray-based cameras (depth_anything_3/utils/ray_utils.py:20-93,313-421, model/da3.py:181-201), forward only: a homography between the
// identity camera's plane grid and the predicted ray directions, fitted per view by confidence-weighted RANSAC, taken apart into rotation, focal lengths
// and principal point.  Upstream sorts, gathers, runs a batched SVD of 16 x 9 matrices, materialises [views, 100, N, 3] projections and refits with a
// full SVD of a [2K, 9] matrix; what that arithmetic amounts to is views x 100 x N point-hypothesis tests and a few 9 x 9 eigenproblems:
//   weights  masked weight per point: conf where |z| of the target ray > z_threshold (strict, in fp32 as torch compares), else 0.  Upstream zeroes these
//            in place in a view of ray_conf, which is how they reach the translation; here the inputs are never written and every kernel reads `wm`
//   fit      one lane per (view, hypothesis): the 8 sampled candidates -> weighted DLT normal matrix -> its smallest eigenvector -> H / H[2,2]
//   score    the only loop over views x hypotheses x points: lanes own points, a view's homographies sit in LDS, per-block partial sums per hypothesis
//   select   partials summed in block order, the largest score wins, the lowest index on a tie (torch.argmax on the CPU)
//   mask     the winner's inliers as a byte mask and their count
//   refit    normal matrix over the kept points, eigenvector, det sign, QL decomposition, translation, [R|T]^-1 and the pixel intrinsics
// The right singular vector of the smallest singular value of the DLT matrix A is the eigenvector of the smallest eigenvalue of A^T A.  Going through
// A^T A squares the condition number (about 1e6 here), so the sums and the cyclic Jacobi solver are fp64; the fp32 inputs are the only fp32 in here and
// every fp32 output is the rounding of an fp64 value.  Both rows of a point carry sqrt(w), so A^T A needs only w and has four distinct symmetric 3 x 3
// blocks with p = (x, y, 1): sum w pp^T (twice on the diagonal), -sum w u pp^T, -sum w v pp^T, sum w (u^2 + v^2) pp^T: 24 sums per problem.
// Every reduction has a fixed order (lane-strided private sums, xor butterfly, waves and blocks in index order; the inlier count is an integer atomic):
// two runs on one input are bit-identical, so a near-tie between two hypotheses cannot change the winner from run to run.
#include "common.h"

#define RP_THREADS 256
#define RP_PPT 4                       // points per lane of the score kernel, lane-strided: one block covers RP_THREADS * RP_PPT points
#define RP_MAX_ITER 128
#define RP_SAMPLES 8
#define RP_FIT_LANES 32                // eigenproblems per block of the fit kernel (2 x 81 doubles of LDS each)
#define RP_MAX_SWEEPS 30

struct RpPoint { double x, y, u, v, w; };

// source point = the plane grid, target = ray[:3] with xy / z where |z| > z_thr (raw xy otherwise; such a point has wm == 0)
__device__ __forceinline__ RpPoint rp_point(const float* __restrict__ ray_v, const float* __restrict__ wm_v, const float* __restrict__ gx,
                                            const float* __restrict__ gy, int p, int pw, float z_thr) {
    const float* r = ray_v + (size_t)p * 6;
    const float rx = r[0], ry = r[1], rz = r[2];
    const bool valid = fabsf(rz) > z_thr;
    RpPoint q;
    q.x = gx[p % pw];
    q.y = gy[p / pw];
    q.u = valid ? (double)rx / (double)rz : (double)rx;
    q.v = valid ? (double)ry / (double)rz : (double)ry;
    q.w = wm_v[p];
    return q;
}

__device__ __forceinline__ void rp_accumulate(double* __restrict__ acc, const RpPoint& q) {
    const double m[6] = {q.x * q.x, q.x * q.y, q.x, q.y * q.y, q.y, 1.0};
    const double s1 = q.w * q.u, s2 = q.w * q.v, s3 = q.w * (q.u * q.u + q.v * q.v);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        acc[i] += q.w * m[i];
        acc[6 + i] += s1 * m[i];
        acc[12 + i] += s2 * m[i];
        acc[18 + i] += s3 * m[i];
    }
}

__device__ __forceinline__ int rp_m6(int i, int j) {          // index of p_i p_j in (xx, xy, x, yy, y, 1)
    const int a = i < j ? i : j, b = i < j ? j : i;
    return a == 0 ? b : (a == 1 ? 2 + b : 5);
}

// A^T A from the 24 sums into A (entry (i, j) at A[(i * 9 + j) * stride]), the identity into Vm
__device__ void rp_build_gram(const double* __restrict__ acc, double* A, double* Vm, int stride) {
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) {
            const int bi = i / 3, bj = j / 3, m = rp_m6(i % 3, j % 3);
            double g = 0.0;
            if (bi == bj) g = bi == 2 ? acc[18 + m] : acc[m];
            else if (bi == 2 || bj == 2) g = -acc[6 * (1 + (bi == 2 ? bj : bi)) + m];
            A[(i * 9 + j) * stride] = g;
            Vm[(i * 9 + j) * stride] = i == j ? 1.0 : 0.0;
        }
}

// cyclic Jacobi on the symmetric 9 x 9 matrix A (destroyed), eigenvectors in the columns of Vm -> h = the eigenvector of the smallest eigenvalue (the lowest
// index on a tie).  One lane per matrix: the rotations of one matrix depend on each other, and the callers have a few hundred matrices at the most.
__device__ void rp_smallest_eigenvector(double* A, double* Vm, int stride, double* __restrict__ h) {
#define RP_A(i, j) A[((i) * 9 + (j)) * stride]
#define RP_V(i, j) Vm[((i) * 9 + (j)) * stride]
    for (int sweep = 0; sweep < RP_MAX_SWEEPS; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 9; ++p) {
            diag += RP_A(p, p) * RP_A(p, p);
            for (int q = p + 1; q < 9; ++q) off += RP_A(p, q) * RP_A(p, q);
        }
        if (!(off > 1e-36 * diag)) break;                      // also leaves on NaN
        for (int p = 0; p < 8; ++p)
            for (int q = p + 1; q < 9; ++q) {
                const double apq = RP_A(p, q);
                if (apq == 0.0) continue;
                const double theta = (RP_A(q, q) - RP_A(p, p)) / (2.0 * apq);
                const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 9; ++k) {
                    const double a = RP_A(k, p), b = RP_A(k, q);
                    RP_A(k, p) = c * a - s * b;
                    RP_A(k, q) = s * a + c * b;
                }
                for (int k = 0; k < 9; ++k) {
                    const double a = RP_A(p, k), b = RP_A(q, k);
                    RP_A(p, k) = c * a - s * b;
                    RP_A(q, k) = s * a + c * b;
                }
                for (int k = 0; k < 9; ++k) {
                    const double a = RP_V(k, p), b = RP_V(k, q);
                    RP_V(k, p) = c * a - s * b;
                    RP_V(k, q) = s * a + c * b;
                }
            }
    }
    int best = 0;
    double lo = RP_A(0, 0);
    for (int i = 1; i < 9; ++i)
        if (RP_A(i, i) < lo) { lo = RP_A(i, i); best = i; }
    for (int k = 0; k < 9; ++k) h[k] = RP_V(k, best);
#undef RP_A
#undef RP_V
}

// reprojection error of q under the row-major homography h: |(Hp)_xy / (Hp)_z - (u, v)|
__device__ __forceinline__ double rp_error(const double* __restrict__ h, const RpPoint& q) {
    const double X = h[0] * q.x + h[1] * q.y + h[2], Y = h[3] * q.x + h[4] * q.y + h[5], Z = h[6] * q.x + h[7] * q.y + h[8];
    const double dx = X / Z - q.u, dy = Y / Z - q.v;
    return sqrt(dx * dx + dy * dy);
}

// The end of a view's refit, one lane: sum = the 24 normal-matrix sums, then sum w and sum w * ray[3:6] over all points.  Eigenvector, H / H[2,2], -A where
// det(A) < 0, A = Q L with a positive diagonal (Gram-Schmidt from the last column, which is the unique factorisation upstream's column-reversed QR plus its
// sign fix arrives at), L / L[2,2], then the inverse of [R|T] and the pixel intrinsics.  sA, sV: 81 doubles each.
__device__ void rp_finish(const double* __restrict__ sum, double* sA, double* sV, double img_h, double img_w, float* __restrict__ H_out,
                          float* __restrict__ R_out, float* __restrict__ T_out, float* __restrict__ focal_out, float* __restrict__ pp_out,
                          float* __restrict__ ext, float* __restrict__ intr) {
    double h[9];
    rp_build_gram(sum, sA, sV, 1);
    rp_smallest_eigenvector(sA, sV, 1, h);
    double A[9];
    for (int k = 0; k < 9; ++k) {
        A[k] = h[k] / h[8];
        H_out[k] = (float)A[k];
    }
    const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    if (det < 0.0)
        for (int k = 0; k < 9; ++k) A[k] = -A[k];
    // columns a0, a1, a2 of A; q2 = a2 / |a2|, q1 from a1 without its q2 part, q0 from a0 without its q1 and q2 parts
    double q0[3], q1[3], q2[3];
    const double l22 = sqrt(A[2] * A[2] + A[5] * A[5] + A[8] * A[8]);
    for (int r = 0; r < 3; ++r) q2[r] = A[r * 3 + 2] / l22;
    const double l21 = q2[0] * A[1] + q2[1] * A[4] + q2[2] * A[7];
    for (int r = 0; r < 3; ++r) q1[r] = A[r * 3 + 1] - l21 * q2[r];
    const double l11 = sqrt(q1[0] * q1[0] + q1[1] * q1[1] + q1[2] * q1[2]);
    for (int r = 0; r < 3; ++r) q1[r] /= l11;
    const double l20 = q2[0] * A[0] + q2[1] * A[3] + q2[2] * A[6];
    for (int r = 0; r < 3; ++r) q0[r] = A[r * 3] - l20 * q2[r];
    const double l10 = q1[0] * q0[0] + q1[1] * q0[1] + q1[2] * q0[2];
    for (int r = 0; r < 3; ++r) q0[r] -= l10 * q1[r];
    const double l00 = sqrt(q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2]);
    for (int r = 0; r < 3; ++r) q0[r] /= l00;
    const double R[9] = {q0[0], q1[0], q2[0], q0[1], q1[1], q2[1], q0[2], q1[2], q2[2]};
    const double T[3] = {sum[25] / sum[24], sum[26] / sum[24], sum[27] / sum[24]};
    const double fx = 1.0 / (l00 / l22), fy = 1.0 / (l11 / l22), px = l20 / l22 + 1.0, py = l21 / l22 + 1.0;
    for (int k = 0; k < 9; ++k) R_out[k] = (float)R[k];
    for (int k = 0; k < 3; ++k) T_out[k] = (float)T[k];
    focal_out[0] = (float)fx; focal_out[1] = (float)fy;
    pp_out[0] = (float)px; pp_out[1] = (float)py;
    float* e = ext;
    for (int r = 0; r < 3; ++r) {                              // [R^T | -R^T T]
        e[r * 4] = (float)R[r]; e[r * 4 + 1] = (float)R[3 + r]; e[r * 4 + 2] = (float)R[6 + r];
        e[r * 4 + 3] = (float)(-((R[r] * T[0] + R[3 + r] * T[1]) + R[6 + r] * T[2]));
    }
    float* k = intr;
    for (int r = 0; r < 9; ++r) k[r] = 0.f;
    k[0] = (float)(fx / 2.0 * img_w);
    k[4] = (float)(fy / 2.0 * img_h);
    k[2] = (float)(px * img_w * 0.5);
    k[5] = (float)(py * img_h * 0.5);
    k[8] = 1.0f;
}

// ---------------------------------------------------------------------------------------------- masked weights
__global__ void da3_ray_weights_kernel(const float* __restrict__ ray, const float* __restrict__ conf, int64_t total, float z_thr, float* __restrict__ wm) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    wm[i] = fabsf(ray[i * 6 + 2]) > z_thr ? conf[i] : 0.f;
}

// ---------------------------------------------------------------------------------------------- hypothesis fit
__global__ __launch_bounds__(64) void da3_ray_fit_kernel(const float* __restrict__ ray, const float* __restrict__ wm, const float* __restrict__ gx,
                                                         const float* __restrict__ gy, const int32_t* __restrict__ cand,
                                                         const int32_t* __restrict__ sample_idx, int n_problems, int n_iter, int n_sample, int N, int pw,
                                                         float z_thr, double* __restrict__ Hs) {
    __shared__ double sA[81 * RP_FIT_LANES], sV[81 * RP_FIT_LANES];
    const int t = threadIdx.x;
    const int id = blockIdx.x * RP_FIT_LANES + t;
    if (t >= RP_FIT_LANES || id >= n_problems) return;         // no barrier below: every lane works on its own matrices
    const int v = id / n_iter, it = id % n_iter;
    double acc[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) acc[i] = 0.0;
    bool ok = true;
    for (int j = 0; j < RP_SAMPLES; ++j) {
        const int si = sample_idx[it * RP_SAMPLES + j];
        if (si < 0 || si >= n_sample) { ok = false; break; }
        const int p = cand[(size_t)v * n_sample + si];
        if (p < 0 || p >= N) { ok = false; break; }
        rp_accumulate(acc, rp_point(ray + (size_t)v * N * 6, wm + (size_t)v * N, gx, gy, p, pw, z_thr));
    }
    double h[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    if (ok) {
        rp_build_gram(acc, sA + t, sV + t, RP_FIT_LANES);
        rp_smallest_eigenvector(sA + t, sV + t, RP_FIT_LANES, h);
    }
    const double h22 = h[8];
    for (int k = 0; k < 9; ++k) Hs[(size_t)id * 9 + k] = ok ? h[k] / h22 : __builtin_nan("");      // an index out of range: a hypothesis nobody fits
}

// ---------------------------------------------------------------------------------------------- scoring
__global__ __launch_bounds__(RP_THREADS) void da3_ray_score_kernel(const float* __restrict__ ray, const float* __restrict__ wm, const float* __restrict__ gx,
                                                                   const float* __restrict__ gy, const double* __restrict__ Hs, int n_iter, int N, int pw,
                                                                   float z_thr, double thr, double* __restrict__ partial) {
    __shared__ double sH[RP_MAX_ITER * 9];
    __shared__ double sP[RP_MAX_ITER][RP_THREADS / 64];
    const int v = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (int i = tid; i < n_iter * 9; i += RP_THREADS) sH[i] = Hs[(size_t)v * n_iter * 9 + i];
    RpPoint q[RP_PPT];
#pragma unroll
    for (int j = 0; j < RP_PPT; ++j) {
        const int64_t p = (int64_t)blockIdx.x * (RP_THREADS * RP_PPT) + j * RP_THREADS + tid;
        if (p < N) q[j] = rp_point(ray + (size_t)v * N * 6, wm + (size_t)v * N, gx, gy, (int)p, pw, z_thr);
        else q[j] = RpPoint{0.0, 0.0, 0.0, 0.0, 0.0};
    }
    __syncthreads();
    for (int h = 0; h < n_iter; ++h) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < RP_PPT; ++j) s += rp_error(sH + h * 9, q[j]) < thr ? q[j].w : 0.0;      // a non-finite error is an outlier, as nan < t
        s = wave_sum(s);
        if (lane == 0) sP[h][wid] = s;
    }
    __syncthreads();
    if (tid < n_iter) {
        double s = 0.0;
        for (int w = 0; w < RP_THREADS / 64; ++w) s += sP[tid][w];
        partial[((size_t)v * gridDim.x + blockIdx.x) * n_iter + tid] = s;
    }
}

// one block per view: scores = partials in block order; the winner; its inlier counter zeroed for the mask kernel
__global__ __launch_bounds__(RP_MAX_ITER) void da3_ray_select_kernel(const double* __restrict__ partial, int nblk, int n_iter, int32_t* __restrict__ best,
                                                                     int32_t* __restrict__ n_inliers) {
    __shared__ double score[RP_MAX_ITER];
    const int v = blockIdx.x, h = threadIdx.x;
    if (h < n_iter) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += partial[((size_t)v * nblk + b) * n_iter + h];
        score[h] = s;
    }
    __syncthreads();
    if (h == 0) {
        int win = 0;
        for (int i = 1; i < n_iter; ++i)
            if (score[i] > score[win]) win = i;
        best[v] = win;
        n_inliers[v] = 0;
    }
}

__global__ __launch_bounds__(RP_THREADS) void da3_ray_mask_kernel(const float* __restrict__ ray, const float* __restrict__ wm, const float* __restrict__ gx,
                                                                  const float* __restrict__ gy, const double* __restrict__ Hs,
                                                                  const int32_t* __restrict__ best, int n_iter, int N, int pw, float z_thr, double thr,
                                                                  uint8_t* __restrict__ inlier, int32_t* __restrict__ n_inliers) {
    const int v = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * RP_THREADS + threadIdx.x;
    const double* hp = Hs + ((size_t)v * n_iter + best[v]) * 9;
    double h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = hp[k];
    bool in = false;
    if (p < N) {
        in = rp_error(h, rp_point(ray + (size_t)v * N * 6, wm + (size_t)v * N, gx, gy, (int)p, pw, z_thr)) < thr;
        inlier[(size_t)v * N + p] = in ? 1 : 0;
    }
    const unsigned long long m = __ballot(in);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_inliers + v, (int)__popcll(m));        // an integer sum: the same in any order
}

// ---------------------------------------------------------------------------------------------- refit, decomposition, cameras
// One block per view.  `use` marks the kept points (the winner's inliers, or the drawn 8000 of them).  T is the mean of ray[3:] under the masked weights of ALL
// points.  Thread 0 finishes (rp_finish).
__global__ __launch_bounds__(RP_THREADS) void da3_ray_refit_kernel(const float* __restrict__ ray, const float* __restrict__ wm, const float* __restrict__ gx,
                                                                   const float* __restrict__ gy, const uint8_t* __restrict__ use, int N, int pw, float z_thr,
                                                                   double img_h, double img_w, float* __restrict__ H_out, float* __restrict__ R_out,
                                                                   float* __restrict__ T_out, float* __restrict__ focal_out, float* __restrict__ pp_out,
                                                                   float* __restrict__ ext, float* __restrict__ intr, int32_t* __restrict__ n_used) {
    __shared__ double red[28][RP_THREADS / 64];
    __shared__ int cnt[RP_THREADS / 64];
    __shared__ double sA[81], sV[81];
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* ray_v = ray + (size_t)v * N * 6;
    const float* wm_v = wm + (size_t)v * N;
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.0;
    int used = 0;
    for (int p = tid; p < N; p += RP_THREADS) {
        const double w = wm_v[p];
        acc[24] += w;
        acc[25] += w * (double)ray_v[(size_t)p * 6 + 3];
        acc[26] += w * (double)ray_v[(size_t)p * 6 + 4];
        acc[27] += w * (double)ray_v[(size_t)p * 6 + 5];
        if (use[(size_t)v * N + p]) {
            rp_accumulate(acc, rp_point(ray_v, wm_v, gx, gy, p, pw, z_thr));
            ++used;
        }
    }
#pragma unroll
    for (int i = 0; i < 28; ++i) {
        const double s = wave_sum(acc[i]);
        if (lane == 0) red[i][wid] = s;
    }
    used = wave_sum(used);
    if (lane == 0) cnt[wid] = used;
    __syncthreads();
    if (tid != 0) return;
    double sum[28];
    for (int i = 0; i < 28; ++i) {
        double s = 0.0;
        for (int w = 0; w < RP_THREADS / 64; ++w) s += red[i][w];
        sum[i] = s;
    }
    int total = 0;
    for (int w = 0; w < RP_THREADS / 64; ++w) total += cnt[w];
    n_used[v] = total;

    rp_finish(sum, sA, sV, img_h, img_w, H_out + v * 9, R_out + v * 9, T_out + v * 3, focal_out + v * 2, pp_out + v * 2, ext + v * 12, intr + v * 9);
}

static bool rp_shape_ok(int64_t V, int64_t ph, int64_t pw) {
    return V > 0 && V <= 65535 && ph > 0 && pw > 0 && ph <= (1 << 15) && pw <= (1 << 15) && ph * pw <= (1 << 26) && V * ph * pw <= 0x7fffffffLL / 6;
}
static int64_t rp_score_blocks(int64_t N) { return (N + RP_THREADS * RP_PPT - 1) / (RP_THREADS * RP_PPT); }

extern "C" {

size_t vgpa_da3_ray_pose_workspace_bytes(int64_t V, int64_t N, int64_t n_iter) {
    if (V <= 0 || N <= 0 || n_iter <= 0 || n_iter > RP_MAX_ITER || V > 65535 || N > (1 << 26)) return 0;
    return (size_t)(V * n_iter * 9 + V * rp_score_blocks(N) * n_iter) * sizeof(double);
}

int32_t vgpa_da3_ray_weights(const float* ray, const float* conf, int64_t V, int64_t N, float z_threshold, float* wm, hipStream_t stream) {
    if (!ray || !conf || !wm || V <= 0 || N <= 0 || V * N > 0x7fffffffLL / 6) return VGPA_ERR_INVALID;
    const int64_t total = V * N;
    VGPA_LAUNCH(da3_ray_weights_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ray, conf, total, z_threshold, wm);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_da3_ray_ransac(const float* ray, const float* wm, const float* gx, const float* gy, const int32_t* cand, const int32_t* sample_idx, int64_t V,
                            int64_t ph, int64_t pw, int64_t n_sample, int64_t n_iter, float z_threshold, double reproj_threshold, int32_t* best,
                            uint8_t* inlier, int32_t* n_inliers, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (!ray || !wm || !gx || !gy || !cand || !sample_idx || !best || !inlier || !n_inliers || !workspace || !rp_shape_ok(V, ph, pw))
        return VGPA_ERR_INVALID;
    const int64_t N = ph * pw;
    if (n_iter <= 0 || n_iter > RP_MAX_ITER || n_sample < RP_SAMPLES || n_sample > N || (reinterpret_cast<uintptr_t>(workspace) & 7u)) return VGPA_ERR_INVALID;
    if (workspace_bytes < vgpa_da3_ray_pose_workspace_bytes(V, N, n_iter)) return VGPA_ERR_WORKSPACE;
    double* Hs = reinterpret_cast<double*>(workspace);
    double* partial = Hs + V * n_iter * 9;
    const int n_problems = (int)(V * n_iter);
    const unsigned nblk = (unsigned)rp_score_blocks(N);
    VGPA_LAUNCH(da3_ray_fit_kernel, dim3((unsigned)((n_problems + RP_FIT_LANES - 1) / RP_FIT_LANES)), dim3(64), 0, stream, ray, wm, gx, gy, cand, sample_idx,
                n_problems, (int)n_iter, (int)n_sample, (int)N, (int)pw, z_threshold, Hs);
    VGPA_CHECK_LAUNCH();
    VGPA_LAUNCH(da3_ray_score_kernel, dim3(nblk, (unsigned)V), dim3(RP_THREADS), 0, stream, ray, wm, gx, gy, Hs, (int)n_iter, (int)N, (int)pw, z_threshold,
                reproj_threshold, partial);
    VGPA_CHECK_LAUNCH();
    VGPA_LAUNCH(da3_ray_select_kernel, dim3((unsigned)V), dim3(RP_MAX_ITER), 0, stream, partial, (int)nblk, (int)n_iter, best, n_inliers);
    VGPA_CHECK_LAUNCH();
    VGPA_LAUNCH(da3_ray_mask_kernel, dim3((unsigned)((N + RP_THREADS - 1) / RP_THREADS), (unsigned)V), dim3(RP_THREADS), 0, stream, ray, wm, gx, gy, Hs, best,
                (int)n_iter, (int)N, (int)pw, z_threshold, reproj_threshold, inlier, n_inliers);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

int32_t vgpa_da3_ray_refit(const float* ray, const float* wm, const float* gx, const float* gy, const uint8_t* use, int64_t V, int64_t ph, int64_t pw,
                           float z_threshold, float image_h, float image_w, float* H, float* R, float* T, float* focal, float* pp, float* ext, float* intr,
                           int32_t* n_used, hipStream_t stream) {
    if (!ray || !wm || !gx || !gy || !use || !H || !R || !T || !focal || !pp || !ext || !intr || !n_used || !rp_shape_ok(V, ph, pw)) return VGPA_ERR_INVALID;
    VGPA_LAUNCH(da3_ray_refit_kernel, dim3((unsigned)V), dim3(RP_THREADS), 0, stream, ray, wm, gx, gy, use, (int)(ph * pw), (int)pw, z_threshold,
                (double)image_h, (double)image_w, H, R, T, focal, pp, ext, intr, n_used);
    VGPA_CHECK_LAUNCH();
    return VGPA_OK;
}

}  // extern "C"
