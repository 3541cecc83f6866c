// ba_tri_refine.hpp — per-point Levenberg-Marquardt refinement of the batched triangulation.
//
// triangulate_reg_kernel (ba_triangulate.hpp) returns the DLT point: the smallest singular vector of the stacked [P_i | -x_i]
// system on UNDISTORTED pixels, an algebraic error.  This kernel starts from that point and minimises the reprojection error
// in the MEASURED pixels,
//     cost(X) = sum_v || uv_v - pi_{c_v}(X) ||^2,
// with pi_c the model of the reference's Camera.project_points(distort=True) (cameras/camera.py:242-272): h = P_c [X; 1],
// pinhole pixel (h0 / h2, h1 / h2), then nb_distort_prealloc (camera.py:32-56) with fx = K00, fy = K11, (cx, cy) = K[0:2, 2] and
// the coefficients [k0, k1, p0, p1, k2] of the camera table (TRI_CAM_STRIDE layout).  P is used as given, K only for the distortion.
//
// Layout as in triangulate_reg_kernel: G lanes per point, lane g owns views g, g + G, ...; the measurement and camera index of its
// first V views stay in registers, further views are re-read from global memory (L2-resident) in every pass; camera rows come from
// the 256-B table (L1-resident).  One pass per LM trial evaluates r and the 2 x 3 Jacobian at the candidate point and accumulates
// 11 sums (6 of H = J'J, 3 of g = J'r, the cost, the number of views with depth h2 <= 0 or a non-finite value); the damped 3 x 3
// system is an LDL' solve with positive-definiteness checked.  An accepted trial's H and g are already summed: a trial costs one pass.
// What a group of lanes guarantees, and the damping, accept and stop rules shared with pnp_lm_kernel: DESIGN.md, "Batched handles".
#pragma once
#include <hip/hip_runtime.h>

#include "ba_device.hpp"
#include "ba_triangulate.hpp"

namespace pcs {

// status codes (include/pcs_hip.h PCS_TRI_REFINE_*)
constexpr int TRI_REFINE_NOT_REFINED = 0;   // non-finite DLT start (fewer than two views included) or a start behind a camera: the DLT point is returned unchanged
constexpr int TRI_REFINE_CONVERGED = 1;     // ftol, xtol or gtol
constexpr int TRI_REFINE_MAX_ITER = 2;      // max_iter trials used
constexpr int TRI_REFINE_NO_DECREASE = 3;   // the damping grew past its limit, or the damped system lost definiteness
constexpr double TRI_REFINE_LAMBDA0 = 1e-4, TRI_REFINE_LAMBDA_MAX = 1e10, TRI_REFINE_LAMBDA_MIN = 1e-15;

// residual r = uv - pi(X) and its Jacobian J = d pi / d X (2 x 3) for one view; `front` = depth h2 > 0
__device__ __forceinline__ void refine_view(const double *__restrict__ ct, const double mu, const double mv, const double X0, const double X1,
                                            const double X2, double &ru, double &rv, double (&J)[2][3], bool &front) {
    const double h0 = fma(ct[0], X0, fma(ct[1], X1, fma(ct[2], X2, ct[3])));
    const double h1 = fma(ct[4], X0, fma(ct[5], X1, fma(ct[6], X2, ct[7])));
    const double h2 = fma(ct[8], X0, fma(ct[9], X1, fma(ct[10], X2, ct[11])));
    front = h2 > 0.0;
    const double iz = tri_rcp(h2);
    const double a = h0 * iz, b = h1 * iz;   // pinhole pixel
    const double fx = ct[22], cx = ct[23], fy = ct[24], cy = ct[25];
    const double k0 = ct[26], k1 = ct[27], p0 = ct[28], p1 = ct[29], k2 = ct[30];
    const double ifx = tri_rcp(fx), ify = tri_rcp(fy);
    const double x = (a - cx) * ifx, y = (b - cy) * ify;
    const double r2 = x * x + y * y;
    const double kup = 1.0 + k0 * r2 + k1 * (r2 * r2) + k2 * (r2 * r2 * r2);
    const double kd = k0 + 2.0 * k1 * r2 + 3.0 * k2 * (r2 * r2);   // d kup / d r2
    const double xD = x * kup + 2.0 * p0 * x * y + p1 * (r2 + 2.0 * (x * x));
    const double yD = y * kup + p0 * (r2 + 2.0 * (y * y)) + 2.0 * p1 * x * y;
    ru = mu - (xD * fx + cx);
    rv = mv - (yD * fy + cy);
    // d(xD, yD) / d(x, y)
    const double cross = 2.0 * x * y * kd + 2.0 * p0 * x + 2.0 * p1 * y;
    const double dxx = kup + 2.0 * x * x * kd + 2.0 * p0 * y + 6.0 * p1 * x;
    const double dyy = kup + 2.0 * y * y * kd + 6.0 * p0 * y + 2.0 * p1 * x;
    // d(u, v) / d(a, b): u = fx xD + cx, x = (a - cx) / fx
    const double ua = dxx, ub = fx * cross * ify, va = fy * cross * ifx, vb = dyy;
    // d(a, b) / dX = (P_0 - a P_2, P_1 - b P_2) / h2
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double da = (ct[k] - a * ct[8 + k]) * iz, db = (ct[4 + k] - b * ct[8 + k]) * iz;
        J[0][k] = ua * da + ub * db;
        J[1][k] = va * da + vb * db;
    }
}

// s: H00 H01 H02 H11 H12 H22 | g0 g1 g2 | cost | bad views
constexpr int TRI_REFINE_SUMS = 11;
__device__ __forceinline__ void refine_accumulate(double (&s)[TRI_REFINE_SUMS], const double ru, const double rv, const double (&J)[2][3], const bool front) {
    s[0] = fma(J[0][0], J[0][0], fma(J[1][0], J[1][0], s[0]));
    s[1] = fma(J[0][0], J[0][1], fma(J[1][0], J[1][1], s[1]));
    s[2] = fma(J[0][0], J[0][2], fma(J[1][0], J[1][2], s[2]));
    s[3] = fma(J[0][1], J[0][1], fma(J[1][1], J[1][1], s[3]));
    s[4] = fma(J[0][1], J[0][2], fma(J[1][1], J[1][2], s[4]));
    s[5] = fma(J[0][2], J[0][2], fma(J[1][2], J[1][2], s[5]));
    s[6] = fma(J[0][0], ru, fma(J[1][0], rv, s[6]));
    s[7] = fma(J[0][1], ru, fma(J[1][1], rv, s[7]));
    s[8] = fma(J[0][2], ru, fma(J[1][2], rv, s[8]));
    s[9] = fma(ru, ru, fma(rv, rv, s[9]));
    s[10] += front ? 0.0 : 1.0;   // behind the camera (NaN depths are not > 0 either)
}

// The robust twin of refine_accumulate: u and v are scaled separately by robust_rho — row s J, residual rho1 f / s — so that
// s[0..6) = sum s^2 J'J, s[6..9) = sum J' rho1 f and s[9] = sum rho0, the cost the loop watches.  `raw` takes the plain sum of
// squares, which the reported RMS needs.
__device__ __forceinline__ void refine_accumulate_robust(double (&s)[TRI_REFINE_SUMS], double &raw, const GroupLoss &loss, const double ru, const double rv,
                                                         const double (&J)[2][3], const bool front) {
    double q0, q1, fu, fv;
    const double su = robust_rho(loss.kind, ru, loss.inv_f_scale, loss.f_scale_sq, q0, fu);
    const double sv = robust_rho(loss.kind, rv, loss.inv_f_scale, loss.f_scale_sq, q1, fv);
    const double S[2][3] = {{su * J[0][0], su * J[0][1], su * J[0][2]}, {sv * J[1][0], sv * J[1][1], sv * J[1][2]}};
    s[0] = fma(S[0][0], S[0][0], fma(S[1][0], S[1][0], s[0]));
    s[1] = fma(S[0][0], S[0][1], fma(S[1][0], S[1][1], s[1]));
    s[2] = fma(S[0][0], S[0][2], fma(S[1][0], S[1][2], s[2]));
    s[3] = fma(S[0][1], S[0][1], fma(S[1][1], S[1][1], s[3]));
    s[4] = fma(S[0][1], S[0][2], fma(S[1][1], S[1][2], s[4]));
    s[5] = fma(S[0][2], S[0][2], fma(S[1][2], S[1][2], s[5]));
    s[6] = fma(S[0][0], fu, fma(S[1][0], fv, s[6]));
    s[7] = fma(S[0][1], fu, fma(S[1][1], fv, s[7]));
    s[8] = fma(S[0][2], fu, fma(S[1][2], fv, s[8]));
    s[9] += q0 + q1;
    s[10] += front ? 0.0 : 1.0;
    raw = fma(ru, ru, fma(rv, rv, raw));
}

// (H + lam diag(H)) d = g by LDL' on the packed upper triangle; false when a pivot is not positive (or not finite)
__device__ __forceinline__ bool refine_solve(const double (&H)[6], const double (&g)[3], const double lam, double (&d)[3]) {
    const double a00 = H[0] * (1.0 + lam), a11 = H[3] * (1.0 + lam), a22 = H[5] * (1.0 + lam);
    const double a01 = H[1], a02 = H[2], a12 = H[4];
    const double D0 = a00;
    const double i0 = tri_rcp(D0);
    const double l10 = a01 * i0, l20 = a02 * i0;
    const double D1 = a11 - l10 * a01;
    const double i1 = tri_rcp(D1);
    const double l21 = (a12 - l20 * a01) * i1;
    const double D2 = a22 - l20 * a02 - l21 * (a12 - l20 * a01);
    const double i2 = tri_rcp(D2);
    const bool pd = D0 > 0.0 && D1 > 0.0 && D2 > 0.0 && D0 < INFINITY && D1 < INFINITY && D2 < INFINITY;
    const double y0 = g[0], y1 = g[1] - l10 * y0, y2 = g[2] - l20 * y0 - l21 * y1;
    d[2] = y2 * i2;
    d[1] = y1 * i1 - l21 * d[2];
    d[0] = y0 * i0 - l10 * d[1] - l20 * d[2];
    return pd && isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]);
}

// The trailing pack is empty (the linear instantiation: the plain sum of squares, signature and code of a kernel that knows no loss;
// profiles/r20/README.md) or (GroupLoss loss, double *cost_out), the robust one: the sums come from refine_accumulate_robust, the cost
// every rule of the loop looks at is sum rho0, the RMS is still the plain one (one more sum per pass), and cost_out (n_pts, 2) receives
// 0.5 sum rho0 at the result and at the start.
template <int G, int V, class... Robust>
__global__ __launch_bounds__(256) void triangulate_refine_kernel(const int32_t *__restrict__ cam, const double2 *__restrict__ uv,
                                                                 const int64_t *__restrict__ start, const double *__restrict__ cam_tab,
                                                                 const double *__restrict__ pts_dlt, int64_t n_pts, const int32_t *__restrict__ order,
                                                                 int max_iter, double ftol, double xtol, double gtol,
                                                                 double *__restrict__ pts_out, double *__restrict__ rms_out, int32_t *__restrict__ info_out,
                                                                 double *__restrict__ resid_out, const Robust... robust) {
    static_assert(is_robust_pack<Robust...>::ok, "the pack is empty (linear) or (GroupLoss, double *cost_out) (robust)");
    constexpr bool ROBUST = sizeof...(Robust) != 0;
    const GroupLoss loss = robust_loss(robust...);
    double *const cost_out = robust_cost_out(robust...);
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    const bool live = gid < n_pts;   // whole groups are live or dead; a dead group never takes part in a pass
    const int64_t jv = live ? gid : n_pts - 1;
    const int64_t j = order ? order[jv] : jv;   // points of equal view counts side by side (tri_order_*_kernel)
    const int64_t s0 = start[j], s1 = live ? start[j + 1] : s0;
    int nv = (int)((s1 - s0 - g + G - 1) / G);
    nv = nv < 0 ? 0 : (nv > V ? V : nv);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nv = max(nv, __shfl_xor(nv, off));
    const int nv_w = __builtin_amdgcn_readfirstlane(nv);   // the wave's largest number of register views per lane (uniform)

    double2 m[V];
    int32_t cm[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        m[v] = make_double2(0.0, 0.0);
        cm[v] = -1;   // absent view
        if (v >= nv_w) continue;
        const int64_t q = s0 + g + (int64_t)v * G;
        if (q < s1) {
            m[v] = uv[q];
            cm[v] = cam[q];
        }
    }
    // one pass: the group's sums at X (every lane of the group gets identical bits)
    auto pass = [&](const double X0, const double X1, const double X2, double (&s)[TRI_REFINE_SUMS], double &raw) {
#pragma unroll
        for (int k = 0; k < TRI_REFINE_SUMS; ++k) s[k] = 0.0;
        if constexpr (ROBUST) raw = 0.0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (v >= nv_w) break;
            if (cm[v] >= 0) {
                double ru, rv, J[2][3];
                bool front;
                refine_view(cam_tab + (int64_t)cm[v] * TRI_CAM_STRIDE, m[v].x, m[v].y, X0, X1, X2, ru, rv, J, front);
                if constexpr (ROBUST) refine_accumulate_robust(s, raw, loss, ru, rv, J, front);
                else refine_accumulate(s, ru, rv, J, front);
            }
        }
        for (int64_t q = s0 + g + (int64_t)V * G; q < s1; q += G) {   // views beyond the registers
            const double2 mq = uv[q];
            double ru, rv, J[2][3];
            bool front;
            refine_view(cam_tab + (int64_t)cam[q] * TRI_CAM_STRIDE, mq.x, mq.y, X0, X1, X2, ru, rv, J, front);
            if constexpr (ROBUST) refine_accumulate_robust(s, raw, loss, ru, rv, J, front);
            else refine_accumulate(s, ru, rv, J, front);
        }
        if constexpr (G > 1) {
#pragma unroll
            for (int k = 0; k < TRI_REFINE_SUMS; ++k) s[k] = group_sum<G>(s[k]);
            if constexpr (ROBUST) raw = group_sum<G>(raw);
        }
    };

    double X[3] = {pts_dlt[3 * j + 0], pts_dlt[3 * j + 1], pts_dlt[3 * j + 2]};
    double H[6] = {0, 0, 0, 0, 0, 0}, gr[3] = {0, 0, 0}, cost = 0.0, cost_dlt = 0.0;
    double raw = 0.0, raw_dlt = 0.0, raw_t = 0.0;   // ROBUST only: the plain sums of squares at the point, at the start and of a trial
    int status = TRI_REFINE_NOT_REFINED, it = 0;
    bool done = !live;
    if (live) {   // the start: cost, H and g at the DLT point
        double s[TRI_REFINE_SUMS];
        pass(X[0], X[1], X[2], s, raw);
        if constexpr (ROBUST) raw_dlt = raw;
#pragma unroll
        for (int k = 0; k < 6; ++k) H[k] = s[k];
        gr[0] = s[6]; gr[1] = s[7]; gr[2] = s[8];
        cost = cost_dlt = s[9];
        const bool ok = isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]) && isfinite(cost) && s[10] == 0.0 && s1 > s0;
        done = !ok;   // not refined: the DLT point is returned unchanged
    }
    double lam = TRI_REFINE_LAMBDA0;
    while (true) {
        double d[3] = {0, 0, 0};
        bool trial = false;
        if (!done) {
            const double gmax = fmax(fabs(gr[0]), fmax(fabs(gr[1]), fabs(gr[2])));
            if (gmax <= gtol) { status = TRI_REFINE_CONVERGED; done = true; }
            else if (it >= max_iter) { status = TRI_REFINE_MAX_ITER; done = true; }
            else if (!refine_solve(H, gr, lam, d)) { status = TRI_REFINE_NO_DECREASE; done = true; }
            else trial = true;
        }
        if (!__any(trial)) break;   // a group's lanes agree; the wave leaves when no group has a trial left
        if (trial) {
            const double T0 = X[0] + d[0], T1 = X[1] + d[1], T2 = X[2] + d[2];
            double s[TRI_REFINE_SUMS];
            pass(T0, T1, T2, s, raw_t);
            ++it;
            const double step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const double size = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
            const bool small = step <= xtol * (xtol + size);
            if (s[10] == 0.0 && s[9] < cost) {   // accepted: lower cost, every view in front (a NaN cost is not lower)
                const bool flat = cost - s[9] <= ftol * cost;
                X[0] = T0; X[1] = T1; X[2] = T2;
#pragma unroll
                for (int k = 0; k < 6; ++k) H[k] = s[k];
                gr[0] = s[6]; gr[1] = s[7]; gr[2] = s[8];
                cost = s[9];
                if constexpr (ROBUST) raw = raw_t;
                lam = fmax(lam * 0.1, TRI_REFINE_LAMBDA_MIN);
                if (flat || small) { status = TRI_REFINE_CONVERGED; done = true; }
            } else {
                lam *= 10.0;
                if (small) { status = TRI_REFINE_CONVERGED; done = true; }   // X is the minimum to within xtol
                else if (lam > TRI_REFINE_LAMBDA_MAX) { status = TRI_REFINE_NO_DECREASE; done = true; }
            }
        }
    }
    if (!live) return;
    // A point with fewer than two views comes with a NaN start (triangulate_kernel) and is not refined.  Its RMS is NaN as well: one
    // view gives a NaN cost, no view gives 0 / 0.  Its loads above are guarded by q < s1, so a point without views reads no observation.
    const double n_v = (double)(s1 - s0);
    if (g == 0) {
        pts_out[3 * j + 0] = X[0];
        pts_out[3 * j + 1] = X[1];
        pts_out[3 * j + 2] = X[2];
        rms_out[2 * j + 0] = sqrt((ROBUST ? raw : cost) / n_v);
        rms_out[2 * j + 1] = sqrt((ROBUST ? raw_dlt : cost_dlt) / n_v);
        if constexpr (ROBUST) {
            // a point that was not refined has the cost of its unchanged start in both; without views NaN, like its RMS (0 / 0)
            cost_out[2 * j + 0] = s1 > s0 ? 0.5 * cost : __builtin_nan("");
            cost_out[2 * j + 1] = s1 > s0 ? 0.5 * cost_dlt : __builtin_nan("");
        }
        info_out[3 * j + 0] = it;
        info_out[3 * j + 1] = status;
        info_out[3 * j + 2] = (int32_t)(s1 - s0);
    }
    if (resid_out) {   // residuals at the returned point, in observation order
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (v >= nv_w) break;
            if (cm[v] >= 0) {
                double ru, rv, J[2][3];
                bool front;
                refine_view(cam_tab + (int64_t)cm[v] * TRI_CAM_STRIDE, m[v].x, m[v].y, X[0], X[1], X[2], ru, rv, J, front);
                const int64_t q = s0 + g + (int64_t)v * G;
                resid_out[2 * q + 0] = ru;
                resid_out[2 * q + 1] = rv;
            }
        }
        for (int64_t q = s0 + g + (int64_t)V * G; q < s1; q += G) {
            const double2 mq = uv[q];
            double ru, rv, J[2][3];
            bool front;
            refine_view(cam_tab + (int64_t)cam[q] * TRI_CAM_STRIDE, mq.x, mq.y, X[0], X[1], X[2], ru, rv, J, front);
            resid_out[2 * q + 0] = ru;
            resid_out[2 * q + 1] = rv;
        }
    }
}

}  // namespace pcs
