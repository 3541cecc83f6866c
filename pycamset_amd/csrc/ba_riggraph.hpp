// ba_riggraph.hpp — view-graph seeding of a rig whose cameras share no commonly seen image.
//
// The reference's estimate_camera_relative_poses (optimisation/template_handler.py:468-601) takes the target of ONE image every camera
// sees as the world and every camera's view of it as its extrinsics; it raises when no such image exists.  Here the extrinsics come from a
// tree through the co-visibility graph, and the per-image candidates are scored in one pass over the detections.  M[c, i] is the view
// transform target -> camera c in image i (the PnP's pose, NaN where there is none); a 3 x 4 transform is 12 doubles, rows [R | t].
//
// rig_view_matrix_kernel — (rotvec, t) -> [R | t] per view (pnp_rodrigues); a pose with a non-finite entry gives twelve NaNs, so that
//   "M[c, i] exists" is "its first entry is not NaN" everywhere below.
// rig_edge_kernel — one workgroup per unordered camera pair (a, b), a < b.  Candidates T_i = M[a, i] inv(M[b, i]) for the images i both
//   see; distance d(T_i, T_j)^2 = (rho^2 / 3) |R_i - R_j|_F^2 + |(R_i - R_j) m_b + t_i - t_j|^2 (|R_i - R_j|_F^2 = 6 - 2 tr(R_i' R_j),
//   formed from the differences: no cancellation), the RMS transfer error over a ball of the target's RMS radius rho about
//   m_b = mean_j M[b, j] pbar.  The pair's transform is the medoid: the candidate of smallest S_i = sum_j d(T_i, T_j), ties to the lowest
//   image.  m_b is summed in image order as well (tiles staged in LDS, one thread adds).  Thread t owns the candidates t, t + 256, ...; the images j are walked in tiles of TILE through LDS, in increasing j, so S_i
//   is the sequential sum in image order whatever the number of images.  d(T_i, T_i) is 0 by definition (not evaluated).  Block
//   reductions (the argmin, the runner-up) are fixed trees over the 256 threads: two runs give the same bits.
// rig_prepare_kernel — W[c, i] = inv(E_c) M[c, i] (camera c's estimate of the target pose of image i in the world of the tree; NaN where
//   M is) and the pre-multiplied projections P_c = K_c E_c of the legacy cost (compiled_helpers.py:518-549).
// rig_score_kernel — one group of G lanes per (view, candidate camera c'): sum over the view's detections of
//   |project_c(P_c [W[c', i] p_k; 1]) - uv| with legacy_cost_kernel's formulas -> partial[c', view]; NaN where W[c', i] is.
// rig_image_sum_kernel — errors[c', i] = the partial sums of image i's views, added in view order (no atomics).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_pnp.hpp"

namespace pcs {

constexpr int RIG_TILE = 64;      // candidates staged through LDS at a time
constexpr int RIG_THREADS = 256;  // threads of an edge workgroup

__global__ __launch_bounds__(256) void rig_view_matrix_kernel(const double *__restrict__ pose, const int64_t n, double *__restrict__ mat) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const double *p = pose + 6 * v;
    const double r[3] = {p[0], p[1], p[2]};
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) fin = fin && isfinite(p[k]);
    double R[9];
    pnp_rodrigues(r, R);
    double *o = mat + 12 * v;
#pragma unroll
    for (int row = 0; row < 3; ++row) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[4 * row + k] = fin ? R[3 * row + k] : __builtin_nan("");
        o[4 * row + 3] = fin ? p[3 + row] : __builtin_nan("");
    }
}

__device__ __forceinline__ bool rig_have(const double *__restrict__ mat, const int64_t v) {
    const double x = mat[12 * v];
    return x == x;
}

// T = A inv(B) for rigid A, B: R = R_a R_b', t = t_a - R t_b
__device__ __forceinline__ void rig_relative(const double *__restrict__ A, const double *__restrict__ B, double (&T)[12]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) T[4 * r + k] = A[4 * r] * B[4 * k] + A[4 * r + 1] * B[4 * k + 1] + A[4 * r + 2] * B[4 * k + 2];
        T[4 * r + 3] = A[4 * r + 3] - (T[4 * r] * B[3] + T[4 * r + 1] * B[7] + T[4 * r + 2] * B[11]);
    }
}

// T = inv(A) B: R = R_a' R_b, t = R_a' (t_b - t_a)
__device__ __forceinline__ void rig_inverse_times(const double *__restrict__ A, const double *__restrict__ B, double (&T)[12]) {
    const double d[3] = {B[3] - A[3], B[7] - A[7], B[11] - A[11]};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k) T[4 * r + k] = A[r] * B[k] + A[4 + r] * B[4 + k] + A[8 + r] * B[8 + k];
        T[4 * r + 3] = A[r] * d[0] + A[4 + r] * d[1] + A[8 + r] * d[2];
    }
}

__device__ __forceinline__ double rig_distance(const double (&Ti)[12], const double *__restrict__ Tj, const double (&m)[3], const double rho2_3) {
    double f = 0.0, e = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double d0 = Ti[4 * r] - Tj[4 * r], d1 = Ti[4 * r + 1] - Tj[4 * r + 1], d2 = Ti[4 * r + 2] - Tj[4 * r + 2];
        f += d0 * d0 + d1 * d1 + d2 * d2;
        const double w = d0 * m[0] + d1 * m[1] + d2 * m[2] + (Ti[4 * r + 3] - Tj[4 * r + 3]);
        e += w * w;
    }
    return sqrt(rho2_3 * f + e);
}

// info (P, 2) = {n, medoid image or -1}; T (P, 12); stats (P, 3) = {sigma, S of the medoid, S of the runner-up (+inf for n < 2)}
template <int TILE>
__global__ __launch_bounds__(RIG_THREADS) void rig_edge_kernel(const double *__restrict__ mat, const int32_t *__restrict__ pair_a,
                                                               const int32_t *__restrict__ pair_b, const int64_t n_imgs, const double c0, const double c1,
                                                               const double c2, const double rho2_3, int32_t *__restrict__ info, double *__restrict__ T_out,
                                                               double *__restrict__ stats) {
    __shared__ double tile[TILE][12];
    __shared__ int tile_ok[TILE];
    __shared__ double red[RIG_THREADS][3];
    __shared__ int red_i[RIG_THREADS];
    const int tid = threadIdx.x;
    const int64_t pair = blockIdx.x;
    const double *Ma = mat + 12 * (int64_t)pair_a[pair] * n_imgs, *Mb = mat + 12 * (int64_t)pair_b[pair] * n_imgs;

    // n and m_b, summed in image order: the images are walked in tiles, the first TILE threads stage M[b, j] pbar of a tile in LDS
    // and thread 0 adds the tile's entries one after the other
    {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        int cnt = 0;
        for (int64_t j0 = 0; j0 < n_imgs; j0 += TILE) {
            __syncthreads();   // thread 0 has read the previous tile
            if (tid < TILE) {
                const int64_t j = j0 + tid;
                const bool ok = j < n_imgs && rig_have(Ma, j) && rig_have(Mb, j);
                tile_ok[tid] = ok;
                if (ok) {
                    const double *B = Mb + 12 * j;
                    tile[tid][0] = B[0] * c0 + B[1] * c1 + B[2] * c2 + B[3];
                    tile[tid][1] = B[4] * c0 + B[5] * c1 + B[6] * c2 + B[7];
                    tile[tid][2] = B[8] * c0 + B[9] * c1 + B[10] * c2 + B[11];
                }
            }
            __syncthreads();
            if (tid == 0)
                for (int jj = 0; jj < TILE; ++jj)
                    if (tile_ok[jj]) { s0 += tile[jj][0]; s1 += tile[jj][1]; s2 += tile[jj][2]; ++cnt; }
        }
        if (tid == 0) { red[0][0] = s0; red[0][1] = s1; red[0][2] = s2; red_i[0] = cnt; }
        __syncthreads();
    }
    const int n = red_i[0];
    const double inv_n = 1.0 / (double)(n > 0 ? n : 1);
    const double m[3] = {red[0][0] * inv_n, red[0][1] * inv_n, red[0][2] * inv_n};
    __syncthreads();   // red is reused below
    if (n == 0) {      // uniform: every thread read the same n
        if (tid == 0) {
            info[2 * pair] = 0; info[2 * pair + 1] = -1;
#pragma unroll
            for (int k = 0; k < 12; ++k) T_out[12 * pair + k] = __builtin_nan("");
            stats[3 * pair] = stats[3 * pair + 1] = stats[3 * pair + 2] = __builtin_nan("");
        }
        return;
    }

    // this thread's best and second-best candidate
    double best = INFINITY, second = INFINITY;
    int best_i = INT32_MAX;
    for (int64_t i0 = 0; i0 < n_imgs; i0 += RIG_THREADS) {   // uniform trip count: the barriers inside are met by every thread
        const int64_t i = i0 + tid;
        const bool mine = i < n_imgs && rig_have(Ma, i) && rig_have(Mb, i);
        double Ti[12];
        if (mine) rig_relative(Ma + 12 * i, Mb + 12 * i, Ti);
        double S = 0.0;
        for (int64_t j0 = 0; j0 < n_imgs; j0 += TILE) {
            __syncthreads();   // the previous tile has been read
            if (tid < TILE) {
                const int64_t j = j0 + tid;
                const bool ok = j < n_imgs && rig_have(Ma, j) && rig_have(Mb, j);
                tile_ok[tid] = ok;
                if (ok) {
                    double Tj[12];
                    rig_relative(Ma + 12 * j, Mb + 12 * j, Tj);
#pragma unroll
                    for (int k = 0; k < 12; ++k) tile[tid][k] = Tj[k];
                }
            }
            __syncthreads();
            if (mine) {
                for (int jj = 0; jj < TILE; ++jj)
                    if (tile_ok[jj] && j0 + jj != i) S += rig_distance(Ti, tile[jj], m, rho2_3);
            }
        }
        if (mine) {   // i grows within a thread: a tie keeps the earlier one
            if (S < best) { second = best; best = S; best_i = (int)i; }
            else if (S < second) second = S;
        }
    }
    red[tid][0] = best; red[tid][1] = second;
    red_i[tid] = best_i;
    __syncthreads();
    for (int h = RIG_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double b0 = red[tid][0], b1 = red[tid + h][0];
            const int i0 = red_i[tid], i1 = red_i[tid + h];
            const bool first = b0 < b1 || (b0 == b1 && i0 <= i1);   // the winner of the two; the loser's best is a runner-up candidate
            const double lose = first ? b1 : b0;
            red[tid][1] = fmin(lose, fmin(red[tid][1], red[tid + h][1]));
            red[tid][0] = first ? b0 : b1;
            red_i[tid] = first ? i0 : i1;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int is = red_i[0];
        info[2 * pair] = n;
        info[2 * pair + 1] = is != INT32_MAX ? is : -1;   // every S non-finite: no medoid
        double T[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) T[k] = __builtin_nan("");
        if (is != INT32_MAX) rig_relative(Ma + 12 * (int64_t)is, Mb + 12 * (int64_t)is, T);
#pragma unroll
        for (int k = 0; k < 12; ++k) T_out[12 * pair + k] = T[k];
        stats[3 * pair] = n > 1 ? red[0][0] / (double)(n - 1) : 0.0;
        stats[3 * pair + 1] = red[0][0];
        stats[3 * pair + 2] = red[0][1];
    }
}

// ext (C, 12) world -> camera; W (C * I, 12); proj (C, 12) = K_c E_c
__global__ __launch_bounds__(256) void rig_prepare_kernel(const double *__restrict__ ext, const double *__restrict__ intr, const double *__restrict__ mat,
                                                          const int64_t n_cams, const int64_t n_imgs, double *__restrict__ W, double *__restrict__ proj) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n_cams) {
        const double *E = ext + 12 * v, *K = intr + 9 * v;
        const double fx = K[0], cx = K[1], fy = K[2], cy = K[3];
        double *P = proj + 12 * v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            P[k] = fx * E[k] + cx * E[8 + k];
            P[4 + k] = fy * E[4 + k] + cy * E[8 + k];
            P[8 + k] = E[8 + k];
        }
    }
    if (v >= n_cams * n_imgs) return;
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = __builtin_nan("");
    if (rig_have(mat, v)) rig_inverse_times(ext + 12 * (v / n_imgs), mat + 12 * v, T);
#pragma unroll
    for (int k = 0; k < 12; ++k) W[12 * v + k] = T[k];
}

template <int G>
__global__ __launch_bounds__(256) void rig_score_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                        const int32_t *__restrict__ view_cam, const int32_t *__restrict__ view_im,
                                                        const double *__restrict__ W, const double *__restrict__ proj, const double *__restrict__ intr,
                                                        const double *__restrict__ pts, const int64_t n_views, const int64_t n_cams, const int64_t n_imgs,
                                                        double *__restrict__ partial) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_views * n_cams) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t view = gid / n_cams, cand = gid % n_cams;   // the candidates of one view side by side: a wave reads one view's detections
    const double *Wc = W + 12 * (cand * n_imgs + view_im[view]);
    double *out = partial + cand * n_views + view;
    if (!(Wc[0] == Wc[0])) {   // the candidate camera has no estimate of this image
        if (g == 0) *out = __builtin_nan("");
        return;
    }
    const int64_t c = view_cam[view];
    double w[12], P[12], cam[9];
#pragma unroll
    for (int k = 0; k < 12; ++k) { w[k] = Wc[k]; P[k] = proj[12 * c + k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) cam[k] = intr[9 * c + k];
    const double fx = cam[0], cx = cam[1], fy = cam[2], cy = cam[3], k0 = cam[4], k1 = cam[5], q0 = cam[6], q1 = cam[7], k2 = cam[8];
    double acc = 0.0;
    for (int64_t o = start[view] + g; o < start[view + 1]; o += G) {
        const double *X = pts + 3 * (int64_t)key[o];
        const double2 m = uv[o];
        const double Y0 = w[0] * X[0] + w[1] * X[1] + w[2] * X[2] + w[3];      // th:535-536: the target's points in the world
        const double Y1 = w[4] * X[0] + w[5] * X[1] + w[6] * X[2] + w[7];
        const double Y2 = w[8] * X[0] + w[9] * X[1] + w[10] * X[2] + w[11];
        double p0 = P[0] * Y0 + P[1] * Y1 + P[2] * Y2 + P[3];                  // ch:538  P [X; 1]
        double p1 = P[4] * Y0 + P[5] * Y1 + P[6] * Y2 + P[7];
        const double p2 = P[8] * Y0 + P[9] * Y1 + P[10] * Y2 + P[11];
        p0 = p0 / p2;                                                          // ch:539
        p1 = p1 / p2;
        const double x = (p0 - cx) / fx, y = (p1 - cy) / fy;                   // ch:455
        const double r2 = x * x + y * y;
        const double kup = 1.0 + k0 * r2 + k1 * (r2 * r2) + k2 * (r2 * r2 * r2);
        const double xD = x * kup + 2.0 * q0 * x * y + q1 * (r2 + 2.0 * x * x);
        const double yD = y * kup + q0 * (r2 + 2.0 * y * y) + 2.0 * q1 * x * y;
        const double eu = (xD * fx + cx) - m.x, ev = (yD * fy + cy) - m.y;     // ch:541-542
        acc += sqrt(eu * eu + ev * ev);                                        // th:545
    }
    if constexpr (G > 1) acc = group_sum<G>(acc);
    if (g == 0) *out = acc;
}

// the views of image i are im_views[im_start[i] .. im_start[i + 1]), in increasing view index
__global__ __launch_bounds__(256) void rig_image_sum_kernel(const double *__restrict__ partial, const int64_t *__restrict__ im_start,
                                                            const int32_t *__restrict__ im_views, const double *__restrict__ W, const int64_t n_cams,
                                                            const int64_t n_imgs, const int64_t n_views, double *__restrict__ errors) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_cams * n_imgs) return;
    const int64_t cand = v / n_imgs, im = v % n_imgs;
    const double w0 = W[12 * v];
    const int64_t q0 = im_start[im], q1 = im_start[im + 1];
    double acc = (w0 == w0 && q1 > q0) ? 0.0 : __builtin_nan("");   // a pose for an image without any view in the table is no candidate
    for (int64_t q = q0; q < q1; ++q) acc += partial[cand * n_views + im_views[q]];
    errors[v] = acc;
}

}  // namespace pcs
