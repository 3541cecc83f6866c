// ba_intr_consensus.hpp — consensus sampling in front of the planar homographies of the intrinsics estimation (opt-in,
// pcs_intr_set_consensus).
//
// What cv2.findHomography(..., RANSAC) is to the plain fit, at the place of AbstractTarget.initial_calibration
// (calibration_targets/abstract_target.py:263-343): one detection with a wrong id is a gross outlier that bends the homography of its
// (camera, image, board) group, and Zhang's constraints of a bent homography lose the camera.  Here H hypotheses per group are fitted to
// sample_size random detections each by the UNCHANGED intr_homography_kernel (ba_intrinsics.hpp) on the pseudo-groups that the UNCHANGED
// pnp_sample_kernel (ba_pnp_consensus.hpp) draws, scored on all detections of the group by a truncated squared transfer error, and the
// unchanged intr_homography_kernel / intr_camera_kernel then run on the table compacted to the winner's inliers (cons_count_scan_kernel,
// cons_compact_kernel; the walks of scoring and selection are those of every consensus stage too, ba_consensus.hpp).  Every group and every (group, hypothesis) is one group of G lanes under the policy of DESIGN.md, "Batched
// handles": xor-butterfly sums (every lane of a group holds identical bits), no floating-point atomics, every sum in a fixed order,
// nothing of a neighbour or of the launch geometry enters a result.  The hypothesis count is fixed: two runs agree bit for bit.
//
// intr_score_kernel   one group of lanes per (group, hypothesis): q = (e1, e2)' (X - c) in the hypothesis' frame, p = H (q, 1),
//                     e^2 = |uv - p_xy / p_z|^2, the score sum min(e^2, tau^2) over the group's observations; tau^2 for a non-finite
//                     measurement or projection and for p_z <= 0 (beyond the plane's horizon); +inf for a hypothesis whose status is not
//                     INTR_GROUP_USED.
// intr_select_kernel  one group of lanes per group: argmin over the H scores (ties: the lower hypothesis), then one flag per
//                     observation, usable and e^2 <= tau^2 at the winner, the inlier count and the number of hypotheses with a finite
//                     homography.  Flagged whole, so that the kernels behind see the group as the plain run does: (a) a group with fewer
//                     observations than max(sample_size, min_points) (consensus not used, score NaN) and (b) a group without a finite
//                     hypothesis (used, score +inf).  (b) differs from the PnP stage on purpose: the group status is a diagnostic
//                     here, and a collinear or non-finite group reports NOT_PLANAR / NOT_FINITE as the plain run does, not TOO_FEW.
// Behind the camera kernel cons_restore_count_kernel puts the observation count of the group back into group_info[:, 1] (the final fit
// wrote the inlier count there, which the camera kernel's pixel centroid has to weight by).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_consensus.hpp"
#include "ba_intrinsics.hpp"

namespace pcs {

// a hypothesis in registers: H (9), then the frame c, e1, e2 (9)
struct IntrHypothesis {
    double H[9], c[3], e1[3], e2[3];
    __device__ __forceinline__ void load(const double *__restrict__ Hh, const double *__restrict__ fr) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = Hh[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { c[k] = fr[k]; e1[k] = fr[3 + k]; e2[k] = fr[6 + k]; }
    }
    // squared transfer error of one observation; `usable`: finite and on the camera's side of the plane's horizon
    __device__ __forceinline__ double e2_of(const double *__restrict__ X, const double2 m, bool &usable) const {
        const double d0 = X[0] - c[0], d1 = X[1] - c[1], d2 = X[2] - c[2];
        const double qx = e1[0] * d0 + e1[1] * d1 + e1[2] * d2, qy = e2[0] * d0 + e2[1] * d1 + e2[2] * d2;
        const double px = H[0] * qx + H[1] * qy + H[2], py = H[3] * qx + H[4] * qy + H[5], pz = H[6] * qx + H[7] * qy + H[8];
        const double ru = m.x - px / pz, rv = m.y - py / pz;
        const double e2 = ru * ru + rv * rv;
        usable = pz > 0.0 && isfinite(e2);
        return e2;
    }
};

// group k = group * H + hypothesis scores the homography hyp_H[k] in its frame hyp_frame[k] on ALL observations of the group -> score[k]
template <int G>
__global__ __launch_bounds__(256) void intr_score_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                         const double *__restrict__ pts, const int64_t n_groups, const int H,
                                                         const double *__restrict__ hyp_H, const double *__restrict__ hyp_frame,
                                                         const int32_t *__restrict__ hyp_info, const double tau2, double *__restrict__ score) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_groups * H) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t j = gid / H;
    const int64_t s0 = start[j], s1 = start[j + 1];
    double s = INFINITY;
    if (hyp_info[2 * gid] == INTR_GROUP_USED) {   // the same in every lane of the group
        IntrHypothesis hyp;
        hyp.load(hyp_H + 9 * gid, hyp_frame + 9 * gid);
        s = cons_truncated_sum<G>(s0, s1, g, tau2, [&](const int64_t o, bool &usable) { return hyp.e2_of(pts + 3 * (int64_t)key[o], uv[o], usable); });
    }
    if (g == 0) score[gid] = s;
}

// cinfo (n_groups, 4): inliers, winning hypothesis (-1: none), hypotheses with a finite homography, consensus used
template <int G>
__global__ __launch_bounds__(256) void intr_select_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                          const double *__restrict__ pts, const int64_t n_groups, const int H, const int n_min,
                                                          const double *__restrict__ hyp_H, const double *__restrict__ hyp_frame,
                                                          const double *__restrict__ score, const double tau2, uint8_t *__restrict__ flag,
                                                          int32_t *__restrict__ cinfo, double *__restrict__ best_out) {
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (j >= n_groups) return;
    const int64_t s0 = start[j], s1 = start[j + 1], n = s1 - s0;
    if (n < n_min) {   // (a) the plain path: every observation goes on
        cons_flag_all<G>(s0, s1, g, flag, 1);
        if (g == 0) {
            cinfo[4 * j + 0] = (int32_t)n; cinfo[4 * j + 1] = -1; cinfo[4 * j + 2] = 0; cinfo[4 * j + 3] = 0;
            best_out[j] = __builtin_nan("");
        }
        return;
    }
    double best;
    int best_k, n_fin;
    cons_argmin<G>(score + j * H, H, g, best, best_k, n_fin, [](int, const double s) { return s < INFINITY; });
    if (best_k == INT32_MAX) {   // (b) no finite hypothesis: this stage alone flags the whole group 1, and the final fit names the reason
        cons_flag_all<G>(s0, s1, g, flag, 1);
        if (g == 0) {
            cinfo[4 * j + 0] = (int32_t)n; cinfo[4 * j + 1] = -1; cinfo[4 * j + 2] = n_fin; cinfo[4 * j + 3] = 1;
            best_out[j] = INFINITY;
        }
        return;
    }
    IntrHypothesis hyp;
    hyp.load(hyp_H + 9 * (j * H + best_k), hyp_frame + 9 * (j * H + best_k));
    const int cnt = cons_flag_inliers<G>(s0, s1, g, tau2, flag,
                                         [&](const int64_t o, bool &usable) { return hyp.e2_of(pts + 3 * (int64_t)key[o], uv[o], usable); });
    if (g == 0) {
        cinfo[4 * j + 0] = cnt; cinfo[4 * j + 1] = best_k; cinfo[4 * j + 2] = n_fin; cinfo[4 * j + 3] = 1;
        best_out[j] = best;
    }
}

}  // namespace pcs
