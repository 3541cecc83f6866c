// ba_align.hpp — batched rigid / similarity registration of 3-D point sets, absolute orientation (pcs_align_run).
//
// What n_estimate_rigid_transform (optimisation/compiled_helpers.py:727-762) does for one pair of point sets by an SVD, here for P
// problems at once: problem j owns rows [start[j], start[j + 1]) of a table of source points x, destination points y and optional
// weights w >= 0, and gets (s, R, t) with y ~ s R x + t in the weighted least-squares sense; s = 1 for the rigid model.  A row with a
// non-finite coordinate or with w = 0 takes no part.  Every problem and every (problem, hypothesis) is one group of G lanes under the
// policy of DESIGN.md, "Batched handles": lane g owns rows g, g + G, ...; xor-butterfly sums (every lane of a group holds identical
// bits); no floating-point atomics, every sum in a fixed order, nothing of a neighbour or of the launch geometry enters a result.
//
// The rotation is Horn's unit quaternion (J. Opt. Soc. Am. A 4, 1987): the eigenvector of the largest eigenvalue of the symmetric
// 4 x 4 matrix N(S), S = sum w x~ y~' on CENTRED coordinates (two passes: target and world coordinates sit far from the origin), by
// cyclic Jacobi (pnp_jacobi<4>).  S is never squared, and a quaternion is a proper rotation by construction: planar sets (sigma_3 = 0)
// and mirror-prone ones (det S < 0) need no special case, unlike pnp_nearest_rotation.  With the eigenvalues l1 >= l2 >= l3 >= l4 of N
// and the singular values of S: l1 = sigma_1 + sigma_2 + d sigma_3 (d = sign det S), so the Umeyama scale is l1 / sum w |x~|^2, and
// (l1 - l2) / (l1 - l4) = (sigma_2 + d sigma_3) / (sigma_1 + sigma_2) tells how well the rotation is determined (0: collinear).
//
// align_fit_kernel<G>      one group per problem, optional per-row mask (the consensus stage's flags): pass 1 sum w and both centroids,
//                          pass 2 S and sum w |x~|^2, closed form, pass 3 weighted RMS of |y - s R x - t| and the per-row distances.
// align_hypothesis_kernel  one thread per (problem, hypothesis): three rows by cons_sample_positions (ba_consensus.hpp; key: the problem index), the same
//                          closed form in registers; [s R | t], NaN for a degenerate or non-finite triple.
// align_score_kernel<G>    one group per (problem, hypothesis): sum min(d^2, tau^2) over all rows; a skipped row counts tau^2; +inf for a
//                          NaN hypothesis.
// align_select_kernel<G>   one group per problem: argmin (ties: the lower hypothesis), one flag per row (d^2 <= tau^2 at the winner), the
//                          inlier count.  A problem of fewer than three rows is flagged whole.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_consensus.hpp"
#include "ba_pnp.hpp"

namespace pcs {

// status codes (include/pcs_hip.h PCS_ALIGN_*)
constexpr int ALIGN_OK = 0;
constexpr int ALIGN_TOO_FEW = 1;        // fewer than min_points usable rows
constexpr int ALIGN_DEGENERATE = 2;     // the conditioning diagnostic is <= rank_tol (collinear or coincident points)
constexpr int ALIGN_NONFINITE = 3;      // every row has a non-finite coordinate, or the fit overflowed
constexpr int ALIGN_NO_CONSENSUS = 4;   // enough usable rows, fewer than min_points inliers
constexpr int ALIGN_SAMPLE = 3;
constexpr int ALIGN_SWEEPS = 10;        // cyclic Jacobi sweeps on the 4 x 4 (quadratic convergence: six reach rounding)

struct AlignRow {
    double x[3], y[3], w;
    bool finite, usable;
};

__device__ __forceinline__ AlignRow align_load(const double *__restrict__ src, const double *__restrict__ dst, const double *__restrict__ wt, const int64_t o) {
    AlignRow r;
    r.finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.x[k] = src[3 * o + k];
        r.y[k] = dst[3 * o + k];
        r.finite = r.finite && isfinite(r.x[k]) && isfinite(r.y[k]);
    }
    r.w = wt ? wt[o] : 1.0;
    r.usable = r.finite && r.w > 0.0;
    return r;
}

// squared distance of a row to the model A = s R (row-major), t
__device__ __forceinline__ double align_d2(const double (&A)[9], const double (&t)[3], const AlignRow &r) {
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double e = r.y[i] - (A[3 * i] * r.x[0] + A[3 * i + 1] * r.x[1] + A[3 * i + 2] * r.x[2]) - t[i];
        d2 += e * e;
    }
    return d2;
}

// The closed form on the sums of a problem: S[3 i + j] = sum w x~_i y~_j, sxx = sum w |x~|^2, the centroids cx, cy.
// -> ALIGN_OK, ALIGN_DEGENERATE or ALIGN_NONFINITE; R, A = s R, t, s and the conditioning diagnostic.
__device__ __forceinline__ int align_closed_form(const double (&S)[9], const double sxx, const double (&cx)[3], const double (&cy)[3], const bool similarity,
                                                 const double rank_tol, double (&R)[9], double (&A)[9], double (&t)[3], double &s, double &cond) {
    double N[4][4], V[4][4];
    N[0][0] = S[0] + S[4] + S[8];
    N[1][1] = S[0] - S[4] - S[8];
    N[2][2] = -S[0] + S[4] - S[8];
    N[3][3] = -S[0] - S[4] + S[8];
    N[0][1] = N[1][0] = S[5] - S[7];
    N[0][2] = N[2][0] = S[6] - S[2];
    N[0][3] = N[3][0] = S[1] - S[3];
    N[1][2] = N[2][1] = S[1] + S[3];
    N[1][3] = N[3][1] = S[6] + S[2];
    N[2][3] = N[3][2] = S[5] + S[7];
    pnp_jacobi<4>(N, V, ALIGN_SWEEPS);
    const double l[4] = {N[0][0], N[1][1], N[2][2], N[3][3]};
    int k1 = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (l[k] > l[k1]) k1 = k;   // ties: the lower index
    double l1 = l[0], l2 = -INFINITY, l4 = l[0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k == k1) {
            l1 = l[k];
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = V[i][k];
        } else {
            l2 = fmax(l2, l[k]);
        }
        l4 = fmin(l4, l[k]);
    }
    cond = (l1 - l2) / (l1 - l4);
    s = similarity ? l1 / sxx : 1.0;
    if (!isfinite(l[0] + l[1] + l[2] + l[3]) || !isfinite(sxx)) {
        cond = __builtin_nan("");
        return ALIGN_NONFINITE;
    }
    if (!(l1 - l4 > 0.0) || !(cond > rank_tol)) {
        if (!(l1 - l4 > 0.0)) cond = 0.0;   // coincident points
        return ALIGN_DEGENERATE;
    }
    const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] * qn, x = q[1] * qn, y = q[2] * qn, z = q[3] * qn;
    R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);         R[7] = 2.0 * (y * z + w * x);         R[8] = w * w - x * x - y * y + z * z;
    bool fin = isfinite(s);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        A[i] = s * R[i];
        fin = fin && isfinite(A[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        t[i] = cy[i] - (A[3 * i] * cx[0] + A[3 * i + 1] * cx[1] + A[3 * i + 2] * cx[2]);
        fin = fin && isfinite(t[i]);
    }
    return fin ? ALIGN_OK : ALIGN_NONFINITE;
}

// T (P, 12) = [R | t] row-major; scale (P); info (P, 4) = [rows used, inliers, status, winning hypothesis or -1]; stats (P, 3) = [weighted
// RMS distance over the rows used, the winner's score (NaN without consensus), conditioning]; dist (rows) the distance of every row to
// the model, or NULL.  Anything but OK has NaN in T, scale, RMS and dist.  mask = NULL: the plain fit, which also writes flag_out (1 where
// the row was used); else the rows with mask != 0, and sel / best (align_select_kernel) go into info and stats.
template <int G>
__global__ __launch_bounds__(256) void align_fit_kernel(const double *__restrict__ src, const double *__restrict__ dst, const double *__restrict__ wt,
                                                        const int64_t *__restrict__ start, const int64_t n_problems, const int similarity,
                                                        const int min_points, const double rank_tol, const uint8_t *__restrict__ mask,
                                                        const int32_t *__restrict__ sel, const double *__restrict__ best, double *__restrict__ T,
                                                        double *__restrict__ scale, int32_t *__restrict__ info, double *__restrict__ stats,
                                                        uint8_t *__restrict__ flag_out, double *__restrict__ dist) {
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (j >= n_problems) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t s0 = start[j], s1 = start[j + 1];
    const double nan = __builtin_nan("");
    // pass 1: sum w, both weighted centroids, the counts
    double sw = 0.0, cx[3] = {0.0, 0.0, 0.0}, cy[3] = {0.0, 0.0, 0.0};
    int n_usable = 0, n_used = 0, n_bad = 0;
    for (int64_t o = s0 + g; o < s1; o += G) {
        const AlignRow r = align_load(src, dst, wt, o);
        const bool used = r.usable && (!mask || mask[o] != 0);
        n_usable += r.usable ? 1 : 0;
        n_bad += r.finite ? 0 : 1;
        if (used) {
            ++n_used;
            sw += r.w;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                cx[k] += r.w * r.x[k];
                cy[k] += r.w * r.y[k];
            }
        }
    }
    sw = group_sum<G>(sw);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cx[k] = group_sum<G>(cx[k]) / sw;
        cy[k] = group_sum<G>(cy[k]) / sw;
    }
    n_usable = group_sum<G>(n_usable);
    n_used = group_sum<G>(n_used);
    n_bad = group_sum<G>(n_bad);
    int status = ALIGN_OK;
    if (n_usable < min_points) status = s1 > s0 && n_bad == s1 - s0 ? ALIGN_NONFINITE : ALIGN_TOO_FEW;
    else if (n_used < min_points) status = ALIGN_NO_CONSENSUS;
    double R[9], A[9], t[3], s = nan, cond = nan, rms = nan;
    if (status == ALIGN_OK) {   // the same in every lane of the group
        // pass 2: cross-covariance and spread of the centred rows
        double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sxx = 0.0;
        for (int64_t o = s0 + g; o < s1; o += G) {
            const AlignRow r = align_load(src, dst, wt, o);
            if (r.usable && (!mask || mask[o] != 0)) {
                const double xc[3] = {r.x[0] - cx[0], r.x[1] - cx[1], r.x[2] - cx[2]};
                const double yc[3] = {r.y[0] - cy[0], r.y[1] - cy[1], r.y[2] - cy[2]};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double wx = r.w * xc[a];
                    sxx += wx * xc[a];
#pragma unroll
                    for (int b = 0; b < 3; ++b) S[3 * a + b] += wx * yc[b];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = group_sum<G>(S[k]);
        sxx = group_sum<G>(sxx);
        status = align_closed_form(S, sxx, cx, cy, similarity != 0, rank_tol, R, A, t, s, cond);
    }
    if (status == ALIGN_OK) {
        // pass 3: the distances of all rows, the weighted RMS over the rows used
        double acc = 0.0;
        for (int64_t o = s0 + g; o < s1; o += G) {
            const AlignRow r = align_load(src, dst, wt, o);
            const bool used = r.usable && (!mask || mask[o] != 0);
            const double d2 = align_d2(A, t, r);
            if (used) acc += r.w * d2;
            if (dist) dist[o] = sqrt(d2);
            if (flag_out) flag_out[o] = used ? 1 : 0;
        }
        rms = sqrt(group_sum<G>(acc) / sw);
        if (!isfinite(rms)) status = ALIGN_NONFINITE;
    }
    if (status != ALIGN_OK) {
        for (int64_t o = s0 + g; o < s1; o += G) {
            if (dist) dist[o] = nan;
            if (flag_out) flag_out[o] = 0;
        }
        s = rms = nan;
    }
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) T[12 * j + 4 * i + k] = status == ALIGN_OK ? R[3 * i + k] : nan;
            T[12 * j + 4 * i + 3] = status == ALIGN_OK ? t[i] : nan;
        }
        scale[j] = s;
        info[4 * j + 0] = n_used;
        info[4 * j + 1] = mask ? sel[3 * j] : n_used;
        info[4 * j + 2] = status;
        info[4 * j + 3] = mask ? sel[3 * j + 1] : -1;
        stats[3 * j + 0] = rms;
        stats[3 * j + 1] = mask ? best[j] : nan;
        stats[3 * j + 2] = cond;
    }
}

// hyp (P H, 12) = [s R | t] of the triple that hypothesis h of problem p draws; NaN for a problem of fewer than three rows, a triple with
// a skipped row, a degenerate or a non-finite one.
__global__ __launch_bounds__(256) void align_hypothesis_kernel(const double *__restrict__ src, const double *__restrict__ dst, const double *__restrict__ wt,
                                                               const int64_t *__restrict__ start, const int64_t n_problems, const int H,
                                                               const uint64_t seed, const int similarity, const double rank_tol,
                                                               double *__restrict__ hyp) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_problems * H) return;
    const int64_t p = k / H;
    const int h = (int)(k - p * H);
    const int64_t s0 = start[p], n = start[p + 1] - s0;
    double R[9], A[9], t[3];
    int status = ALIGN_TOO_FEW;
    if (n >= ALIGN_SAMPLE) {
        int64_t pick[CONS_MAX_SAMPLE];
        cons_sample_positions(seed, (int32_t)p, n, h, ALIGN_SAMPLE, pick);
        AlignRow r[ALIGN_SAMPLE];
        bool usable = true;
        double sw = 0.0, cx[3] = {0.0, 0.0, 0.0}, cy[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < ALIGN_SAMPLE; ++i) {
            r[i] = align_load(src, dst, wt, s0 + pick[i]);
            usable = usable && r[i].usable;
            sw += r[i].w;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                cx[c] += r[i].w * r[i].x[c];
                cy[c] += r[i].w * r[i].y[c];
            }
        }
        if (usable) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                cx[c] /= sw;
                cy[c] /= sw;
            }
            double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, sxx = 0.0;
#pragma unroll
            for (int i = 0; i < ALIGN_SAMPLE; ++i) {
                const double xc[3] = {r[i].x[0] - cx[0], r[i].x[1] - cx[1], r[i].x[2] - cx[2]};
                const double yc[3] = {r[i].y[0] - cy[0], r[i].y[1] - cy[1], r[i].y[2] - cy[2]};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double wx = r[i].w * xc[a];
                    sxx += wx * xc[a];
#pragma unroll
                    for (int b = 0; b < 3; ++b) S[3 * a + b] += wx * yc[b];
                }
            }
            double s, cond;
            status = align_closed_form(S, sxx, cx, cy, similarity != 0, rank_tol, R, A, t, s, cond);
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) hyp[12 * k + i] = status == ALIGN_OK ? A[i] : __builtin_nan("");
#pragma unroll
    for (int i = 0; i < 3; ++i) hyp[12 * k + 9 + i] = status == ALIGN_OK ? t[i] : __builtin_nan("");
}

__device__ __forceinline__ bool align_load_hypothesis(const double *__restrict__ h, double (&A)[9], double (&t)[3]) {
    bool fin = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        A[i] = h[i];
        fin = fin && isfinite(A[i]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        t[i] = h[9 + i];
        fin = fin && isfinite(t[i]);
    }
    return fin;
}

template <int G>
__global__ __launch_bounds__(256) void align_score_kernel(const double *__restrict__ src, const double *__restrict__ dst, const double *__restrict__ wt,
                                                          const int64_t *__restrict__ start, const int64_t n_problems, const int H,
                                                          const double *__restrict__ hyp, const double tau2, double *__restrict__ score) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_problems * H) return;
    const int64_t p = gid / H;
    const int64_t s0 = start[p], s1 = start[p + 1];
    double A[9], t[3], sum = INFINITY;
    if (align_load_hypothesis(hyp + 12 * gid, A, t)) {   // the same in every lane of the group
        sum = cons_truncated_sum<G>(s0, s1, g, tau2, [&](const int64_t o, bool &usable) {
            const AlignRow r = align_load(src, dst, wt, o);
            usable = r.usable;
            return align_d2(A, t, r);
        });
    }
    if (g == 0) score[gid] = sum;
}

// sel (P, 3): inliers, winning hypothesis (-1: none), consensus used; best: the winner's score (+inf: no usable hypothesis, NaN: fewer
// than three rows, consensus not used)
template <int G>
__global__ __launch_bounds__(256) void align_select_kernel(const double *__restrict__ src, const double *__restrict__ dst, const double *__restrict__ wt,
                                                           const int64_t *__restrict__ start, const int64_t n_problems, const int H,
                                                           const double *__restrict__ hyp, const double *__restrict__ score, const double tau2,
                                                           uint8_t *__restrict__ flag, int32_t *__restrict__ sel, double *__restrict__ best_out) {
    const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (p >= n_problems) return;
    const int64_t s0 = start[p], s1 = start[p + 1], n = s1 - s0;
    if (n < ALIGN_SAMPLE) {   // the plain path: every row goes on
        cons_flag_all<G>(s0, s1, g, flag, 1);
        if (g == 0) {
            sel[3 * p + 0] = (int32_t)n; sel[3 * p + 1] = -1; sel[3 * p + 2] = 0;
            best_out[p] = __builtin_nan("");
        }
        return;
    }
    double best;
    int best_k, n_fin;
    cons_argmin<G>(score + p * H, H, g, best, best_k, n_fin, cons_count_none);
    if (best_k == INT32_MAX) {   // no finite hypothesis: no inlier
        cons_flag_all<G>(s0, s1, g, flag, 0);
        if (g == 0) {
            sel[3 * p + 0] = 0; sel[3 * p + 1] = -1; sel[3 * p + 2] = 1;
            best_out[p] = INFINITY;
        }
        return;
    }
    double A[9], t[3];
    align_load_hypothesis(hyp + 12 * (p * H + best_k), A, t);
    const int cnt = cons_flag_inliers<G>(s0, s1, g, tau2, flag, [&](const int64_t o, bool &usable) {
        const AlignRow r = align_load(src, dst, wt, o);
        usable = r.usable;
        return align_d2(A, t, r);
    });
    if (g == 0) {
        sel[3 * p + 0] = cnt; sel[3 * p + 1] = best_k; sel[3 * p + 2] = 1;
        best_out[p] = best;
    }
}

}  // namespace pcs
