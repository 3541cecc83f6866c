// ba_pnp_consensus.hpp — consensus sampling in front of the batched target-pose estimation (opt-in, pcs_pnp_set_consensus).
//
// What cv2.solvePnPRansac is to cv2.solvePnPGeneric, at the place of AbstractTarget.target_pose_in_cam_image
// (calibration_targets/abstract_target.py:345-405): one detection with a wrong id is a gross outlier that bends the linear start of its
// view.  Here H hypotheses per view are fitted to sample_size random detections each by the UNCHANGED pnp_start_kernel (ba_pnp.hpp), scored
// on all detections of the view by a truncated squared error, and the unchanged pnp_start_kernel / pnp_lm_kernel then run on the table
// compacted to the winner's inliers.  Every view and every (view, hypothesis) is one group of G lanes under the policy of DESIGN.md,
// "Batched handles": xor-butterfly sums (every lane of a group holds identical bits), no floating-point atomics, every sum in a fixed
// order, nothing of a neighbour or of the launch geometry enters a result.  The hypothesis count is fixed: two runs agree bit for bit.
//
// The generator, the walks of scoring and selection, and the scan, compaction and restored-count kernels are those of every consensus
// stage (ba_consensus.hpp); here is what belongs to the target pose.
//
// pnp_sample_kernel   one thread per (view, hypothesis): sample_size distinct positions inside the view by cons_sample_positions, keyed
//                     by (seed, camera, observations of the view, hypothesis); positions ascending; the sampled (key, uv) rows become a
//                     pseudo-view of sample_size observations.  The view's rows arrive sorted by key, so the same table shuffled draws
//                     the same detections.
//                     A view with fewer observations than sample_size gets NaN rows (its hypotheses are NaN and never looked at).
// pnp_score_kernel    one group per (view, hypothesis): sum min(e^2, tau^2) over the view's observations for the start and for the second
//                     pose of the planar ambiguity in ONE walk, full Brown-Conrady projection (pnp_point); tau^2 for a non-finite
//                     measurement or projection and for a depth <= 0; +inf for a non-finite candidate.  RESID = true is the one-candidate
//                     mode: the residuals of all observations of a view at a given pose (NaN where the pose is NaN).
// pnp_select_kernel   one group per view: argmin over the 2 H scores (ties: the lower hypothesis, then the first pose before the second),
//                     then one flag per observation, e^2 <= tau^2 at the winner, the inlier count and the number of hypotheses with a
//                     finite candidate.  A view with fewer observations than sample_size is flagged whole (consensus not used); a view
//                     without a finite candidate has no inlier.  Too few inliers for min_points: the kernels behind refuse the view.
// Behind them cons_count_scan_kernel and cons_compact_kernel<16> make the table of the flagged rows, and cons_restore_count_kernel puts
// the observation count of the view back into info[2] (the LM wrote the inlier count there).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_consensus.hpp"
#include "ba_pnp.hpp"

namespace pcs {

__global__ __launch_bounds__(256) void pnp_sample_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                         const int32_t *__restrict__ view_cam, const int64_t n_views, const int H, const int S,
                                                         const uint64_t seed, int32_t *__restrict__ s_key, double2 *__restrict__ s_uv,
                                                         int64_t *__restrict__ s_start, int32_t *__restrict__ s_vcam) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_views * H) return;
    const int64_t j = k / H;
    const int h = (int)(k - j * H);
    const int64_t s0 = start[j], n = start[j + 1] - s0;
    const int32_t cam = view_cam[j];
    s_vcam[k] = cam;
    s_start[k] = k * S;
    if (k == n_views * H - 1) s_start[k + 1] = (k + 1) * S;
    int32_t *ok = s_key + k * S;
    double2 *ouv = s_uv + k * S;
    if (n < S) {   // not sampled: a pseudo-view that pnp_start_kernel answers with NaN
        for (int i = 0; i < S; ++i) {
            ok[i] = 0;
            ouv[i] = make_double2(__builtin_nan(""), __builtin_nan(""));
        }
        return;
    }
    int64_t pick[CONS_MAX_SAMPLE];
    cons_sample_positions(seed, cam, n, h, S, pick);
#pragma unroll
    for (int i = 0; i < CONS_MAX_SAMPLE; ++i)
        if (i < S) {
            ok[i] = key[s0 + pick[i]];
            ouv[i] = uv[s0 + pick[i]];
        }
}

// squared pixel error of one observation at (R, t); `usable`: finite and in front of the camera
__device__ __forceinline__ double pnp_consensus_e2(const double (&R)[9], const double (&t)[3], const double (&cam)[9], const double *__restrict__ X,
                                                   const double2 m, double &ru, double &rv, bool &usable) {
    double Ju[6], Jv[6];
    bool front;
    pnp_point(R, t, cam, X[0], X[1], X[2], m.x, m.y, ru, rv, Ju, Jv, front);
    const double e2 = ru * ru + rv * rv;
    usable = front && isfinite(e2);
    return e2;
}

__device__ __forceinline__ bool pnp_load_pose(const double *__restrict__ p, double (&R)[9], double (&t)[3]) {
    bool fin = true;
    double ps[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        ps[k] = p[k];
        fin = fin && isfinite(ps[k]);
    }
    const double r[3] = {ps[0], ps[1], ps[2]};
    pnp_rodrigues(r, R);
    t[0] = ps[3]; t[1] = ps[4]; t[2] = ps[5];
    return fin;
}

// RESID = false: group k = view * H + hypothesis scores pose_a[k] and pose_b[k] -> score[2 k], score[2 k + 1].
// RESID = true (H = 1): group j writes the residuals of view j at pose_a[j] to resid_out, in observation order.
template <int G, bool RESID>
__global__ __launch_bounds__(256) void pnp_score_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                        const int32_t *__restrict__ view_cam, const double *__restrict__ cam_tab,
                                                        const double *__restrict__ pts, const int64_t n_views, const int H,
                                                        const double *__restrict__ pose_a, const double *__restrict__ pose_b, const double tau2,
                                                        double *__restrict__ score, double *__restrict__ resid_out) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_views * H) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t j = gid / H;
    const int64_t s0 = start[j], s1 = start[j + 1];
    double cam[9];
    {
        const double *ct = cam_tab + (int64_t)view_cam[j] * TRI_CAM_STRIDE + 22;
#pragma unroll
        for (int k = 0; k < 9; ++k) cam[k] = ct[k];
    }
    double Ra[9], ta[3];
    const bool fin_a = pnp_load_pose(pose_a + 6 * gid, Ra, ta);
    if constexpr (RESID) {
        for (int64_t o = s0 + g; o < s1; o += G) {
            double ru, rv;
            bool usable;
            pnp_consensus_e2(Ra, ta, cam, pts + 3 * (int64_t)key[o], uv[o], ru, rv, usable);
            resid_out[2 * o + 0] = fin_a ? ru : __builtin_nan("");
            resid_out[2 * o + 1] = fin_a ? rv : __builtin_nan("");
        }
    } else {
        double Rb[9], tb[3];
        const bool fin_b = pnp_load_pose(pose_b + 6 * gid, Rb, tb) && fin_a;
        double sa = 0.0, sb = 0.0;
        if (fin_a) {   // the same in every lane of the group
            for (int64_t o = s0 + g; o < s1; o += G) {
                const double2 m = uv[o];
                const double *X = pts + 3 * (int64_t)key[o];
                double ru, rv;
                bool usable;
                const double ea = pnp_consensus_e2(Ra, ta, cam, X, m, ru, rv, usable);
                sa += usable && ea <= tau2 ? ea : tau2;
                if (fin_b) {
                    const double eb = pnp_consensus_e2(Rb, tb, cam, X, m, ru, rv, usable);
                    sb += usable && eb <= tau2 ? eb : tau2;
                }
            }
            sa = group_sum<G>(sa);
            sb = group_sum<G>(sb);
        }
        if (g == 0) {
            score[2 * gid + 0] = fin_a ? sa : INFINITY;
            score[2 * gid + 1] = fin_b ? sb : INFINITY;
        }
    }
}

// cinfo (n_views, 4): inliers, winning hypothesis (-1: none), hypotheses with a finite candidate, consensus used
template <int G>
__global__ __launch_bounds__(256) void pnp_select_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                         const int32_t *__restrict__ view_cam, const double *__restrict__ cam_tab,
                                                         const double *__restrict__ pts, const int64_t n_views, const int H, const int S,
                                                         const double *__restrict__ pose_a, const double *__restrict__ pose_b,
                                                         const double *__restrict__ score, const double tau2, uint8_t *__restrict__ flag,
                                                         int32_t *__restrict__ cinfo, double *__restrict__ best_out) {
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (j >= n_views) return;
    const int64_t s0 = start[j], s1 = start[j + 1], n = s1 - s0;
    if (n < S) {   // the plain path: every observation goes on
        cons_flag_all<G>(s0, s1, g, flag, 1);
        if (g == 0) {
            cinfo[4 * j + 0] = (int32_t)n; cinfo[4 * j + 1] = -1; cinfo[4 * j + 2] = 0; cinfo[4 * j + 3] = 0;
            best_out[j] = __builtin_nan("");
        }
        return;
    }
    double best;
    int best_k, n_fin;   // candidate 2 h + c is pose c of hypothesis h: a hypothesis counts once, by its first pose
    cons_argmin<G>(score + 2 * j * H, 2 * H, g, best, best_k, n_fin, [](const int k, const double s) { return !(k & 1) && s < INFINITY; });
    if (best_k == INT32_MAX) {   // no finite candidate: no inlier, the kernels behind refuse the empty view
        cons_flag_all<G>(s0, s1, g, flag, 0);
        if (g == 0) {
            cinfo[4 * j + 0] = 0; cinfo[4 * j + 1] = -1; cinfo[4 * j + 2] = n_fin; cinfo[4 * j + 3] = 1;
            best_out[j] = INFINITY;
        }
        return;
    }
    double cam[9], R[9], t[3];
    {
        const double *ct = cam_tab + (int64_t)view_cam[j] * TRI_CAM_STRIDE + 22;
#pragma unroll
        for (int k = 0; k < 9; ++k) cam[k] = ct[k];
    }
    pnp_load_pose(((best_k & 1) ? pose_b : pose_a) + 6 * (j * H + (best_k >> 1)), R, t);
    const int cnt = cons_flag_inliers<G>(s0, s1, g, tau2, flag, [&](const int64_t o, bool &usable) {
        double ru, rv;
        return pnp_consensus_e2(R, t, cam, pts + 3 * (int64_t)key[o], uv[o], ru, rv, usable);
    });
    if (g == 0) {
        cinfo[4 * j + 0] = cnt; cinfo[4 * j + 1] = best_k >> 1; cinfo[4 * j + 2] = n_fin; cinfo[4 * j + 3] = 1;
        best_out[j] = best;
    }
}

}  // namespace pcs
