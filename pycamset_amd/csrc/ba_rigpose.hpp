// ba_rigpose.hpp — the target pose of every image in a calibrated rig.
//
// The reference's find_target_pose_at_timestep / find_target_poses (optimisation/find_target.py:9-82) fix every camera's extrinsics,
// intrinsics and distortion and run the whole bundle adjustment for the poses that are left.  With the cameras fixed that problem is
// block diagonal: one 6-parameter least-squares problem per image over the detections of ALL cameras that see it.  Here every image is
// one group of G lanes; what such a group guarantees is in DESIGN.md, "Batched handles".
//
// rigpose_lm_kernel<G> — Levenberg-Marquardt on the measured pixels, full Brown-Conrady model.  Unknown T_i = (R, t), target -> world;
//   residual of a detection (c, i, k): uv - project_c(E_c (R X_k + t)) with E_c = [Re | te] world -> camera c (the convention of
//   rig_score_kernel).  Update R <- exp([d omega]x) R, t <- t + d t: d X_cam = Re (-[R X]x d omega + d t).  An observation is evaluated
//   with pnp_point at the "pose" (Re, te) of its camera and the WORLD point R X + t, which gives a = d pixel / d X_cam; the row of the
//   Jacobian is [(R X) x (Re' a), Re' a].  One pass per trial accumulates the 21 + 6 + 2 sums of PNP_SUMS; damping, accept and stop rules
//   are those of pnp_lm_kernel ("The group-LM kernels"), a point counts as behind when it is behind ITS camera.
//   Lane g owns observations g, g + G, ... of the image's run.  No observation stays in registers between passes: the camera differs per
//   observation, so what a pass needs per observation is 9 intrinsics + 12 extrinsics + 3 template coordinates + 2 pixels through two
//   indices; keeping the 5 doubles that do not depend on the camera would save 2 of 6 loads and cost 5 V registers per lane.  The tables
//   (C x 21 doubles, K x 3) stay in L2 / the vector cache.
//   A pose that no accepted trial moved is returned with the bits of its start.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_pnp.hpp"

namespace pcs {

constexpr int RIGPOSE_EXT_STRIDE = 12;   // rows [Re | te] of a 3 x 4 transform
constexpr int RIGPOSE_HESS = 21;         // packed upper triangle of H by rows, the first 21 of PNP_SUMS

// one observation of camera c at the image pose (R, t): residual and Jacobian rows with respect to (d omega, d t) of the IMAGE pose
__device__ __forceinline__ void rigpose_point(const double (&R)[9], const double (&t)[3], const double *__restrict__ ct, const double *__restrict__ e,
                                              const double *__restrict__ X, const double2 m, double &ru, double &rv, double (&Ju)[6], double (&Jv)[6],
                                              bool &front) {
    const double cam[9] = {ct[0], ct[1], ct[2], ct[3], ct[4], ct[5], ct[6], ct[7], ct[8]};
    const double Re[9] = {e[0], e[1], e[2], e[4], e[5], e[6], e[8], e[9], e[10]}, te[3] = {e[3], e[7], e[11]};
    const double X0 = X[0], X1 = X[1], X2 = X[2];
    const double Y0 = fma(R[0], X0, fma(R[1], X1, R[2] * X2)), Y1 = fma(R[3], X0, fma(R[4], X1, R[5] * X2)), Y2 = fma(R[6], X0, fma(R[7], X1, R[8] * X2));
    double Jcu[6], Jcv[6];
    pnp_point(Re, te, cam, Y0 + t[0], Y1 + t[1], Y2 + t[2], m.x, m.y, ru, rv, Jcu, Jcv, front);
    // a = d pixel / d X_cam is the translation part of the camera-frame rows; to the world frame: Re' a
    const double a0 = Re[0] * Jcu[3] + Re[3] * Jcu[4] + Re[6] * Jcu[5], a1 = Re[1] * Jcu[3] + Re[4] * Jcu[4] + Re[7] * Jcu[5],
                 a2 = Re[2] * Jcu[3] + Re[5] * Jcu[4] + Re[8] * Jcu[5];
    const double b0 = Re[0] * Jcv[3] + Re[3] * Jcv[4] + Re[6] * Jcv[5], b1 = Re[1] * Jcv[3] + Re[4] * Jcv[4] + Re[7] * Jcv[5],
                 b2 = Re[2] * Jcv[3] + Re[5] * Jcv[4] + Re[8] * Jcv[5];
    Ju[0] = Y1 * a2 - Y2 * a1; Ju[1] = Y2 * a0 - Y0 * a2; Ju[2] = Y0 * a1 - Y1 * a0; Ju[3] = a0; Ju[4] = a1; Ju[5] = a2;
    Jv[0] = Y1 * b2 - Y2 * b1; Jv[1] = Y2 * b0 - Y0 * b2; Jv[2] = Y0 * b1 - Y1 * b0; Jv[3] = b0; Jv[4] = b1; Jv[5] = b2;
}

// The trailing pack is empty (the linear instantiation: the plain sum of squares, signature and code of a kernel that knows no loss;
// profiles/r20/README.md) or (GroupLoss loss, double *cost_out), the robust one: the sums come from pnp_accumulate_robust, so the cost
// every rule of the loop looks at (accept, ftol, usable start) is sum rho0, gtol looks at the robust g and hess_out receives the robust
// H; the RMS is still the plain one (one more sum per pass), and cost_out (n_imgs, 2) receives 0.5 sum rho0 at the result and at the
// start (NaN where no pose was estimated).
template <int G, class... Robust>
__global__ __launch_bounds__(256) void rigpose_lm_kernel(const int32_t *__restrict__ key, const int32_t *__restrict__ cam, const double2 *__restrict__ uv,
                                                         const int64_t *__restrict__ start, const double *__restrict__ cam_tab,
                                                         const double *__restrict__ ext_tab, const double *__restrict__ pts, const int64_t n_imgs,
                                                         const int32_t *__restrict__ order, const double *__restrict__ pose_start, const int max_iter,
                                                         const double ftol, const double xtol, const double gtol, const int min_points,
                                                         double *__restrict__ pose_out, double *__restrict__ rms_out, int32_t *__restrict__ info_out,
                                                         double *__restrict__ hess_out, double *__restrict__ resid_out, const Robust... robust) {
    static_assert(is_robust_pack<Robust...>::ok, "the pack is empty (linear) or (GroupLoss, double *cost_out) (robust)");
    constexpr bool ROBUST = sizeof...(Robust) != 0;
    const GroupLoss loss = robust_loss(robust...);
    double *const cost_out = robust_cost_out(robust...);
    static_assert(G == 16 || G == 32 || G == 64, "a group is a power-of-two part of one wave");
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    const bool live = gid < n_imgs;   // whole groups are live or dead; a dead group never takes part in a pass
    const int64_t jv = live ? gid : n_imgs - 1;
    const int64_t j = order ? order[jv] : jv;
    const int64_t s0 = start[j], s1 = live ? start[j + 1] : s0;
    const int64_t n = s1 - s0;
    const bool enough = live && n > 0 && n >= min_points;

    // one pass: the group's sums at (R, t) (every lane of the group gets identical bits)
    auto pass = [&](const double (&R)[9], const double (&t)[3], double (&s)[PNP_SUMS], double &raw) {
#pragma unroll
        for (int k = 0; k < PNP_SUMS; ++k) s[k] = 0.0;
        if constexpr (ROBUST) raw = 0.0;
        for (int64_t q = s0 + g; q < s1; q += G) {
            const int64_t c = cam[q];
            double ru, rv, Ju[6], Jv[6];
            bool front;
            rigpose_point(R, t, cam_tab + c * TRI_CAM_STRIDE + 22, ext_tab + c * RIGPOSE_EXT_STRIDE, pts + 3 * (int64_t)key[q], uv[q], ru, rv, Ju, Jv, front);
            if constexpr (ROBUST) pnp_accumulate_robust(s, raw, loss, ru, rv, Ju, Jv, front);
            else pnp_accumulate(s, ru, rv, Ju, Jv, front);
        }
#pragma unroll
        for (int k = 0; k < PNP_SUMS; ++k) s[k] = group_sum<G>(s[k]);
        if constexpr (ROBUST) raw = group_sum<G>(raw);
    };

    // cameras that contribute: the runs of the (non-decreasing) camera column inside the image
    double heads = 0.0;
    for (int64_t q = s0 + g; q < s1; q += G) heads += (q == s0 || cam[q] != cam[q - 1]) ? 1.0 : 0.0;
    heads = group_sum<G>(heads);

    double ps[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) ps[k] = pose_start[6 * j + k];
    bool fin = enough;
#pragma unroll
    for (int k = 0; k < 6; ++k) fin = fin && isfinite(ps[k]);
    double R[9], t[3] = {ps[3], ps[4], ps[5]}, cur[PNP_SUMS], cost0 = 0.0;
    double raw = 0.0, raw0 = 0.0, raw_t = 0.0;   // ROBUST only: the plain sums of squares at the pose, at the start and of a trial
    {
        const double r[3] = {ps[0], ps[1], ps[2]};
        pnp_rodrigues(r, R);
    }
#pragma unroll
    for (int k = 0; k < PNP_SUMS; ++k) cur[k] = 0.0;
    int status = PNP_NOT_ESTIMATED, it = 0;
    bool done = true, moved = false;
    if (fin) {   // cost, H and g at the start
        pass(R, t, cur, raw);
        cost0 = cur[27];
        if constexpr (ROBUST) raw0 = raw;
        done = !(isfinite(cur[27]) && cur[28] == 0.0);   // not estimated from this start
    }
    const bool usable = !done;
    double lam = PNP_LAMBDA0;
    while (true) {
        double d[6] = {0, 0, 0, 0, 0, 0};
        bool trial = false;
        if (!done) {
            double gmax = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) gmax = fmax(gmax, fabs(cur[21 + k]));
            if (gmax <= gtol) { status = PNP_CONVERGED; done = true; }
            else if (it >= max_iter) { status = PNP_MAX_ITER; done = true; }
            else if (!pnp_solve(cur, lam, d)) { status = PNP_NO_DECREASE; done = true; }
            else trial = true;
        }
        if (!__any(trial)) break;   // a group's lanes agree; the wave leaves when no group has a trial left
        if (trial) {
            const double w[3] = {d[0], d[1], d[2]};
            double dR[9], Rt[9], s[PNP_SUMS];
            pnp_rodrigues(w, dR);
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) Rt[3 * r + k] = dR[3 * r] * R[k] + dR[3 * r + 1] * R[3 + k] + dR[3 * r + 2] * R[6 + k];
            const double tt[3] = {t[0] + d[3], t[1] + d[4], t[2] + d[5]};
            pass(Rt, tt, s, raw_t);
            ++it;
            const double step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
            const double size = sqrt(3.0 + t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);   // Frobenius size of [R | t]
            const bool small = step <= xtol * (xtol + size);
            if (s[28] == 0.0 && s[27] < cur[27]) {   // accepted: lower cost, every point in front of its camera (a NaN cost is not lower)
                const bool flat = cur[27] - s[27] <= ftol * cur[27];
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = Rt[k];
                t[0] = tt[0]; t[1] = tt[1]; t[2] = tt[2];
#pragma unroll
                for (int k = 0; k < PNP_SUMS; ++k) cur[k] = s[k];
                moved = true;
                if constexpr (ROBUST) raw = raw_t;
                lam = fmax(lam * 0.1, PNP_LAMBDA_MIN);
                if (flat || small) { status = PNP_CONVERGED; done = true; }
            } else {
                lam *= 10.0;
                if (small) { status = PNP_CONVERGED; done = true; }
                else if (lam > PNP_LAMBDA_MAX) { status = PNP_NO_DECREASE; done = true; }
            }
        }
    }
    if (!live) return;
    const bool est = usable && status != PNP_NOT_ESTIMATED;
    double best[6];
    if (est && moved) {
        double rv[3];
        pnp_rotvec(R, rv);
        best[0] = rv[0]; best[1] = rv[1]; best[2] = rv[2];
        best[3] = t[0]; best[4] = t[1]; best[5] = t[2];
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) best[k] = est ? ps[k] : __builtin_nan("");   // never moved: the start's bits
    }
    if (g == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) pose_out[6 * j + k] = best[k];
        const double inv_n = 1.0 / (double)n;
        rms_out[2 * j + 0] = est ? sqrt((ROBUST ? raw : cur[27]) * inv_n) : __builtin_nan("");
        rms_out[2 * j + 1] = est ? sqrt((ROBUST ? raw0 : cost0) * inv_n) : __builtin_nan("");
        if constexpr (ROBUST) {
            cost_out[2 * j + 0] = est ? 0.5 * cur[27] : __builtin_nan("");
            cost_out[2 * j + 1] = est ? 0.5 * cost0 : __builtin_nan("");
        }
        info_out[4 * j + 0] = est ? it : 0;
        info_out[4 * j + 1] = est ? status : PNP_NOT_ESTIMATED;
        info_out[4 * j + 2] = (int32_t)n;
        info_out[4 * j + 3] = (int32_t)heads;
#pragma unroll
        for (int k = 0; k < RIGPOSE_HESS; ++k) hess_out[RIGPOSE_HESS * j + k] = est ? cur[k] : __builtin_nan("");
    }
    if (resid_out) {   // residuals at the returned pose, in observation order (NaN where no pose was estimated)
        double Rb[9];
        const double r[3] = {best[0], best[1], best[2]}, tb[3] = {best[3], best[4], best[5]};
        pnp_rodrigues(r, Rb);
        for (int64_t q = s0 + g; q < s1; q += G) {
            const int64_t c = cam[q];
            double ru, rv, Ju[6], Jv[6];
            bool front;
            rigpose_point(Rb, tb, cam_tab + c * TRI_CAM_STRIDE + 22, ext_tab + c * RIGPOSE_EXT_STRIDE, pts + 3 * (int64_t)key[q], uv[q], ru, rv, Ju, Jv, front);
            resid_out[2 * q + 0] = est ? ru : __builtin_nan("");
            resid_out[2 * q + 1] = est ? rv : __builtin_nan("");
        }
    }
}

}  // namespace pcs
