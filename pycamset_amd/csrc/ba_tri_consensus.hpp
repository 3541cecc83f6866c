// ba_tri_consensus.hpp — view-pair consensus in front of the batched triangulation (opt-in, pcs_tri_set_consensus).
//
// What the two-view RANSAC of COLMAP's and OpenCV's n-view triangulation is to their DLT, at the place of nb_triangulate_full
// (compiled_helpers.py:609-643): one mismatched view is a gross outlier that drags the DLT start of its point, and the refinement starts
// there.  Here H hypotheses per point are triangulated from PAIRS of its views by the UNCHANGED triangulation kernel of the handle
// (ba_triangulate.hpp), scored on all views of the point by a truncated squared reprojection error in the measured pixels (refine_view
// of ba_tri_refine.hpp: full Brown-Conrady), and the unchanged triangulate_* / triangulate_refine_kernel then run on the table compacted
// to the winner's inliers.  Every point and every (point, hypothesis) is one group of G lanes under the policy of DESIGN.md, "Batched
// handles": xor-butterfly sums (every lane of a group holds identical bits), no floating-point atomics, every sum in a fixed order,
// nothing of a neighbour or of the launch geometry enters a result.  The hypothesis count is fixed: two runs agree bit for bit.
//
// tri_cons_used_kernel     one thread per point: how many of its H hypotheses are used — 0 below three views (the plain path),
//                          min(H, V (V - 1) / 2) otherwise — into cinfo[4 j]; cons_count_scan_kernel (ba_consensus.hpp) turns them into
//                          the row bases of the pseudo-table (integers).
// tri_sample_kernel        one thread per (point, hypothesis): a pair of view positions a < b.  V (V - 1) / 2 <= H: all pairs in
//                          lexicographic order, the hypotheses beyond the last pair unused.  Otherwise one 64-bit draw r of the counter-based
//                          generator of ba_consensus.hpp (cons_mix64) keyed by (seed, point index, V, hypothesis): a = r mod V,
//                          b = (r >> 32) mod (V - 1) bumped past a; duplicate pairs are allowed.  The two (camera, uv) rows become a
//                          pseudo-point of two views; an unused hypothesis repeats its start index, which the triangulation kernels answer
//                          with three NaNs.
// tri_score_kernel         one group per (point, hypothesis): sum min(e^2, tau^2) over the point's views; tau^2 for a non-finite
//                          measurement or projection and for a depth <= 0; +inf for a non-finite candidate.  RESID = true is the
//                          one-candidate mode: the residuals of all observations of a point at a given point (NaN where the point is NaN).
// tri_select_kernel        one group per point: argmin over the H scores (ties: the lower hypothesis), then one flag per observation,
//                          e^2 <= tau^2 at the winner with depth > 0, the inlier count and the number of finite hypotheses.  Fewer than
//                          three views: flagged whole (consensus not used).  No finite candidate, or fewer than two inliers: no row is
//                          kept and the kernels behind write NaN.
// Behind them cons_count_scan_kernel again and cons_compact_kernel<4> make the table of the flagged rows (the order inside a point is
// kept), and cons_restore_count_kernel puts the full view count of the point back into info[2] (the refinement wrote the inlier count
// there).  The walks of scoring and selection are those of every consensus stage (ba_consensus.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_consensus.hpp"
#include "ba_tri_refine.hpp"

namespace pcs {

constexpr int TRI_CONS_MIN_VIEWS = 3;   // below: two views have one pair and nothing to vote with

// hypotheses of a point with V views that carry a pair
__host__ __device__ __forceinline__ int64_t tri_cons_used(const int64_t V, const int H) {
    if (V < TRI_CONS_MIN_VIEWS) return 0;
    const int64_t pairs = V * (V - 1) / 2;   // V < 2^31 (an int32 camera per row): no overflow
    return pairs <= (int64_t)H ? pairs : (int64_t)H;
}

__global__ __launch_bounds__(256) void tri_cons_used_kernel(const int64_t *__restrict__ start, const int64_t n_pts, const int H, int32_t *__restrict__ cinfo) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_pts) return;
    cinfo[4 * j] = (int32_t)tri_cons_used(start[j + 1] - start[j], H);
}

// the pair of hypothesis h of point j with V >= 3 views: positions a < b in [0, V)
__device__ __forceinline__ void tri_cons_pair(const uint64_t seed, const int64_t j, const int64_t V, const int H, const int h, int64_t &a, int64_t &b) {
    if (V * (V - 1) / 2 <= (int64_t)H) {   // exhaustive: pair h in lexicographic order (V <= 23 here: at most 22 steps)
        int64_t rem = h;
        a = 0;
        while (rem >= V - 1 - a) {
            rem -= V - 1 - a;
            ++a;
        }
        b = a + 1 + rem;
        return;
    }
    uint64_t k = cons_mix64(seed + CONS_GOLDEN);
    k = cons_mix64(k ^ (uint64_t)j);
    k = cons_mix64(k ^ (uint64_t)V);
    k = cons_mix64(k ^ (uint64_t)(uint32_t)h);
    const uint64_t r = cons_mix64(k + CONS_GOLDEN);
    const int64_t p = (int64_t)(r % (uint64_t)V);
    int64_t q = (int64_t)((r >> 32) % (uint64_t)(V - 1));
    q += q >= p ? 1 : 0;
    a = p < q ? p : q;
    b = p < q ? q : p;
}

// h_base (n_pts + 1): exclusive scan of the used counts.  Hypothesis k = j H + h has its two rows at 2 (h_base[j] + h); s_start (n_pts H + 1).
__global__ __launch_bounds__(256) void tri_sample_kernel(const int32_t *__restrict__ cam, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                         const int64_t *__restrict__ h_base, const int64_t n_pts, const int H, const uint64_t seed,
                                                         int32_t *__restrict__ s_cam, double2 *__restrict__ s_uv, int64_t *__restrict__ s_start) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pts * H) return;
    const int64_t j = k / H;
    const int h = (int)(k - j * H);
    const int64_t s0 = start[j], V = start[j + 1] - s0;
    const int64_t used = tri_cons_used(V, H), base = h_base[j];
    s_start[k] = 2 * (base + ((int64_t)h < used ? (int64_t)h : used));
    if (k == n_pts * H - 1) s_start[k + 1] = 2 * (base + used);
    if ((int64_t)h >= used) return;   // unused: its start index repeats the next one's
    int64_t a, b;
    tri_cons_pair(seed, j, V, H, h, a, b);
    const int64_t row = 2 * (base + h);
    s_cam[row] = cam[s0 + a];
    s_uv[row] = uv[s0 + a];
    s_cam[row + 1] = cam[s0 + b];
    s_uv[row + 1] = uv[s0 + b];
}

// squared pixel error of one observation at X; `usable`: finite and in front of the camera
__device__ __forceinline__ double tri_consensus_e2(const double *__restrict__ cam_tab, const int32_t c, const double2 m, const double X0, const double X1,
                                                   const double X2, double &ru, double &rv, bool &usable) {
    double J[2][3];
    bool front;
    refine_view(cam_tab + (int64_t)c * TRI_CAM_STRIDE, m.x, m.y, X0, X1, X2, ru, rv, J, front);
    const double e2 = ru * ru + rv * rv;
    usable = front && isfinite(e2);
    return e2;
}

// RESID = false: group k = point * H + hypothesis scores cand[k] -> score[k].
// RESID = true (H = 1): group j writes the residuals of point j at cand[j] to resid_out, in observation order.
template <int G, bool RESID>
__global__ __launch_bounds__(256) void tri_score_kernel(const int32_t *__restrict__ cam, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                        const double *__restrict__ cam_tab, const int64_t n_pts, const int H,
                                                        const double *__restrict__ cand, const double tau2, double *__restrict__ score,
                                                        double *__restrict__ resid_out) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pts * H) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t j = gid / H;
    const int64_t s0 = start[j], s1 = start[j + 1];
    const double X0 = cand[3 * gid + 0], X1 = cand[3 * gid + 1], X2 = cand[3 * gid + 2];
    const bool fin = isfinite(X0) && isfinite(X1) && isfinite(X2);   // the same in every lane of the group
    if constexpr (RESID) {
        for (int64_t o = s0 + g; o < s1; o += G) {
            double ru, rv;
            bool usable;
            tri_consensus_e2(cam_tab, cam[o], uv[o], X0, X1, X2, ru, rv, usable);
            resid_out[2 * o + 0] = fin ? ru : __builtin_nan("");
            resid_out[2 * o + 1] = fin ? rv : __builtin_nan("");
        }
    } else {
        double sum = INFINITY;
        if (fin)
            sum = cons_truncated_sum<G>(s0, s1, g, tau2, [&](const int64_t o, bool &usable) {
                double ru, rv;
                return tri_consensus_e2(cam_tab, cam[o], uv[o], X0, X1, X2, ru, rv, usable);
            });
        if (g == 0) score[gid] = sum;
    }
}

// cinfo (n_pts, 4): inliers, winning hypothesis (-1: none), finite hypotheses, consensus used
template <int G>
__global__ __launch_bounds__(256) void tri_select_kernel(const int32_t *__restrict__ cam, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                         const double *__restrict__ cam_tab, const int64_t n_pts, const int H,
                                                         const double *__restrict__ cand, const double *__restrict__ score, const double tau2,
                                                         uint8_t *__restrict__ flag, int32_t *__restrict__ cinfo, double *__restrict__ best_out) {
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (j >= n_pts) return;
    const int64_t s0 = start[j], s1 = start[j + 1], V = s1 - s0;
    if (V < TRI_CONS_MIN_VIEWS) {   // the plain path: every observation goes on
        cons_flag_all<G>(s0, s1, g, flag, 1);
        if (g == 0) {
            cinfo[4 * j + 0] = (int32_t)(V < 0 ? 0 : V); cinfo[4 * j + 1] = -1; cinfo[4 * j + 2] = 0; cinfo[4 * j + 3] = 0;
            best_out[j] = __builtin_nan("");
        }
        return;
    }
    double best;
    int best_k, n_fin;
    cons_argmin<G>(score + j * H, H, g, best, best_k, n_fin, [](int, const double s) { return s < INFINITY; });
    if (best_k == INT32_MAX) {   // no finite candidate: no row is kept, the kernels behind write NaN
        cons_flag_all<G>(s0, s1, g, flag, 0);
        if (g == 0) {
            cinfo[4 * j + 0] = 0; cinfo[4 * j + 1] = -1; cinfo[4 * j + 2] = n_fin; cinfo[4 * j + 3] = 1;
            best_out[j] = INFINITY;
        }
        return;
    }
    const double *X = cand + 3 * (j * H + best_k);
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    const auto e2_of = [&](const int64_t o, bool &usable) {
        double ru, rv;
        return tri_consensus_e2(cam_tab, cam[o], uv[o], X0, X1, X2, ru, rv, usable);
    };
    // This stage alone counts before it flags: one row determines no point, so nothing is kept of a winner with fewer than two inliers.
    const int cnt = cons_flag_inliers<G>(s0, s1, g, tau2, (uint8_t *)nullptr, e2_of);
    const bool keep = cnt >= 2;
    if (keep) cons_flag_inliers<G>(s0, s1, g, tau2, flag, e2_of);
    else cons_flag_all<G>(s0, s1, g, flag, 0);
    if (g == 0) {
        cinfo[4 * j + 0] = keep ? cnt : 0; cinfo[4 * j + 1] = best_k; cinfo[4 * j + 2] = n_fin; cinfo[4 * j + 3] = 1;
        best_out[j] = best;
    }
}

}  // namespace pcs
