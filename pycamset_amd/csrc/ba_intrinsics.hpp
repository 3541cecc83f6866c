// ba_intrinsics.hpp — camera intrinsics from planar target views.
//
// The rough intrinsics the reference's calc_initial_params starts from: AbstractTarget.initial_calibration
// (calibration_targets/abstract_target.py:263-343) collects, per camera, every (image, board) group with more than 12 detections and
// hands them to cv2.calibrateCamera.  Here the closed form of that call: Zhang's method with zero skew and, where the image size is
// known, OpenCV's initCameraMatrix2D (principal point at the image centre, focal lengths only).  Derivation, degeneracies and the
// model-selection rule: DESIGN.md section 4, "Intrinsics from planar views".  Two kernels:
//
// intr_homography_kernel — one group of G lanes per (camera, image, board) group, in the style of pnp_start_kernel:
//   centroid c, scatter and plane frame (e1, e2) of the group's template points with the PnP start's routines and planarity rule;
//   plane coordinates q = (e1, e2)' (X - c) / s; measured pixels normalised by Hartley's rule (their centroid, mean distance sqrt 2:
//   no undistortion, the camera is unknown); homography with h33 = 1 by the 8 x 8 normal equations (pnp_fit<2>); written
//   de-normalised, pixels <- metric plane frame, with the frame (c, e1, e2) beside it: the in-plane axes of a square grid are any
//   orthogonal pair, so a homography is comparable only together with its frame.
// intr_camera_kernel — one group of G lanes per camera, the lanes striding over the camera's USED groups (contiguous after the host sort):
//   H <- N H with N = [[1/s0, 0, -c0x/s0], [0, 1/s0, -c0y/s0], [0, 0, 1]]; (h1, h2) scaled jointly by 1 / sqrt((|h1|^2 + |h2|^2) / 2), which
//   does not depend on the choice of the in-plane axes (|h1| |h2| does, and a square grid leaves that choice to rounding); the two
//   constraints h1' B h2 = 0 and (h1' B h1 - h2' B h2) / 2 = 0 on b = (B11, B22, B13, B23, B33) give two rows of V per group (the
//   half makes a rotation of the in-plane axes by theta a rotation of the two rows by 2 theta, so V'V does not depend on the axes
//   either); the 15 sums of V'V are taken per lane and combined in a fixed order.  Full model: the eigenvector of the smallest eigenvalue (cyclic Jacobi on
//   5 x 5).  Focal model: B13 = B23 = 0, B33 = 1, which leaves the 2 x 2 block of the same sums.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_pnp.hpp"

namespace pcs {

// per-group status (include/pcs_hip.h PCS_INTR_GROUP_*)
constexpr int INTR_GROUP_TOO_FEW = 0;      // fewer than min_points observations
constexpr int INTR_GROUP_USED = 1;
constexpr int INTR_GROUP_NOT_PLANAR = 2;   // the template points of the group do not lie in a plane (or on a line)
constexpr int INTR_GROUP_NOT_FINITE = 3;   // a non-finite measurement, or every measurement in one pixel
constexpr int INTR_GROUP_FIT_FAILED = 4;   // the normal equations of the homography lost definiteness
// per-camera status (PCS_INTR_*) and models (PCS_INTR_MODEL_*; "auto" is resolved by the host)
constexpr int INTR_NOT_ESTIMATED = 0, INTR_FULL = 1, INTR_FOCAL = 2, INTR_FOCAL_FALLBACK = 3;
constexpr int INTR_MODEL_FULL = 1, INTR_MODEL_FOCAL = 2;
constexpr int INTR_JACOBI_SWEEPS = 12;
// V'V has a null space of more than one dimension when its second smallest eigenvalue is rounding against its largest: B is then
// not determined (one view, or views that are all parallel to the image plane).  The same figure bounds the focal system's determinant.
constexpr double INTR_RANK_TOL = 1e-12;

// measurement -> Hartley-normalised pixel: (m - centroid) * sqrt 2 / mean distance
struct IntrHartleyMap {
    double mu, mv, k;
    __device__ __forceinline__ void operator()(const double2 m, double &x, double &y) const {
        x = (m.x - mu) * k;
        y = (m.y - mv) * k;
    }
};

template <int G>
__global__ __launch_bounds__(256) void intr_homography_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                              const double *__restrict__ pts, const int64_t n_groups, const int min_points,
                                                              double *__restrict__ H_out, double *__restrict__ frame_out, int32_t *__restrict__ info_out,
                                                              double *__restrict__ pix_out) {
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (j >= n_groups) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t s0 = start[j], s1 = start[j + 1];
    const int64_t n = s1 - s0;
    int status = INTR_GROUP_USED;
    double H[9], fr[9], px[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = fr[k] = __builtin_nan("");
    px[0] = px[1] = px[2] = __builtin_nan("");
    if (n <= 0 || n < min_points) {
        status = INTR_GROUP_TOO_FEW;
    } else {
        double c[3], e1[3], e2[3], e3[3], l_min, l_mid, s;
        pnp_template_frame<G>(key, pts, s0, s1, g, n, c, e1, e2, e3, l_min, l_mid, s);
        // centroid of the measured pixels, then their mean distance from it
        const double inv_n = 1.0 / (double)n;
        double mu = 0.0, mv = 0.0, d = 0.0;
        for (int64_t o = s0 + g; o < s1; o += G) {
            const double2 m = uv[o];
            mu += m.x; mv += m.y;
        }
        mu = group_sum<G>(mu) * inv_n;
        mv = group_sum<G>(mv) * inv_n;
        for (int64_t o = s0 + g; o < s1; o += G) {
            const double2 m = uv[o];
            const double dx = m.x - mu, dy = m.y - mv;
            d += sqrt(dx * dx + dy * dy);
        }
        d = group_sum<G>(d) * inv_n;
        px[0] = mu; px[1] = mv; px[2] = d;
        if (!(isfinite(mu) && isfinite(mv) && d > 0.0 && d < INFINITY)) status = INTR_GROUP_NOT_FINITE;
        else if (!(l_min < PNP_PLANAR_RATIO * l_mid)) status = INTR_GROUP_NOT_PLANAR;
        if (status == INTR_GROUP_USED) {   // the group's lanes agree
            const double F[2][3] = {{e1[0], e1[1], e1[2]}, {e2[0], e2[1], e2[2]}};
            const double inv_s = 1.0 / s;
            const IntrHartleyMap map{mu, mv, sqrt(2.0) / d};
            double h[8];
            const bool ok = pnp_fit<2, G>(key, uv, s0, s1, g, map, pts, c, F, inv_s, h);
            // pixels <- plane frame in metres: T^-1 [h] diag(1/s, 1/s, 1), T^-1 = [[1/k, 0, mu], [0, 1/k, mv], [0, 0, 1]]
            const double ik = d / sqrt(2.0);
            H[0] = (ik * h[0] + mu * h[6]) * inv_s; H[1] = (ik * h[1] + mu * h[7]) * inv_s; H[2] = ik * h[2] + mu;
            H[3] = (ik * h[3] + mv * h[6]) * inv_s; H[4] = (ik * h[4] + mv * h[7]) * inv_s; H[5] = ik * h[5] + mv;
            H[6] = h[6] * inv_s;                    H[7] = h[7] * inv_s;                    H[8] = 1.0;
            bool fin = ok;
#pragma unroll
            for (int k = 0; k < 9; ++k) fin = fin && isfinite(H[k]);
            if (!fin) {
                status = INTR_GROUP_FIT_FAILED;
#pragma unroll
                for (int k = 0; k < 9; ++k) H[k] = __builtin_nan("");
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) { fr[k] = c[k]; fr[3 + k] = e1[k]; fr[6 + k] = e2[k]; }
            }
        }
    }
    if (g == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) { H_out[9 * j + k] = H[k]; frame_out[9 * j + k] = fr[k]; }
#pragma unroll
        for (int k = 0; k < 3; ++k) pix_out[3 * j + k] = px[k];
        info_out[2 * j + 0] = status;
        info_out[2 * j + 1] = (int32_t)n;
    }
}

// the row of V for the pair (a, c): a' B c = v . (B11, B22, B13, B23, B33) with B12 = 0
__device__ __forceinline__ void intr_constraint(const double (&a)[3], const double (&c)[3], double (&v)[5]) {
    v[0] = a[0] * c[0];
    v[1] = a[1] * c[1];
    v[2] = a[0] * c[2] + a[2] * c[0];
    v[3] = a[1] * c[2] + a[2] * c[1];
    v[4] = a[2] * c[2];
}

template <int G>
__global__ __launch_bounds__(256) void intr_camera_kernel(const double *__restrict__ H, const int32_t *__restrict__ group_info, const double *__restrict__ pix,
                                                          const int64_t *__restrict__ cam_start, const double *__restrict__ res, const int64_t n_cams,
                                                          const int model, double *__restrict__ intr_out, int32_t *__restrict__ info_out,
                                                          double *__restrict__ eig_out) {
    const int64_t cam = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (cam >= n_cams) return;   // whole groups leave together
    const int64_t g0 = cam_start[cam], g1 = cam_start[cam + 1];
    // groups used, and the count-weighted mean of their pixel centroids and spreads
    double used = 0.0, w = 0.0, wx = 0.0, wy = 0.0, wd = 0.0;
    // Lane g takes the used groups number g, g + G, ... of the camera, counted among the USED ones: a group that drops out (a NaN
    // measurement) leaves the sums what they are without it, bit for bit.  Every lane walks the camera's statuses for that, twice:
    // one 4-byte load per group and pass, the same address in all 16 lanes (one request per group of lanes), against 72 bytes and
    // some 150 FMAs for a group a lane takes; at rig-32's 1 200 groups per camera that is 10 KB per camera from L2.
    int u = 0;
    for (int64_t j = g0; j < g1; ++j) {
        if (group_info[2 * j] != INTR_GROUP_USED) continue;
        if ((u++ & (G - 1)) != g) continue;
        const double nj = (double)group_info[2 * j + 1];
        used += 1.0;
        w += nj;
        wx = fma(nj, pix[3 * j], wx); wy = fma(nj, pix[3 * j + 1], wy); wd = fma(nj, pix[3 * j + 2], wd);
    }
    used = group_sum<G>(used); w = group_sum<G>(w); wx = group_sum<G>(wx); wy = group_sum<G>(wy); wd = group_sum<G>(wd);
    double c0x = wx / w, c0y = wy / w, sc = wd / w;
    if (res) {   // (h, w) of the camera: the image centre and the mean side
        const double rh = res[2 * cam], rw = res[2 * cam + 1];
        c0x = 0.5 * (rw - 1.0); c0y = 0.5 * (rh - 1.0); sc = 0.5 * (rw + rh);
    }
    const int n_used = (int)used;
    double out[4], ratio = __builtin_nan("");
    out[0] = out[1] = out[2] = out[3] = __builtin_nan("");
    int status = INTR_NOT_ESTIMATED;
    if (n_used > 0) {   // the group's lanes agree
        const double is = 1.0 / sc;
        double M[15];
#pragma unroll
        for (int k = 0; k < 15; ++k) M[k] = 0.0;
        u = 0;
        for (int64_t j = g0; j < g1; ++j) {
            if (group_info[2 * j] != INTR_GROUP_USED) continue;
            if ((u++ & (G - 1)) != g) continue;
            const double *Hj = H + 9 * j;
            double h1[3] = {(Hj[0] - c0x * Hj[6]) * is, (Hj[3] - c0y * Hj[6]) * is, Hj[6]};
            double h2[3] = {(Hj[1] - c0x * Hj[7]) * is, (Hj[4] - c0y * Hj[7]) * is, Hj[7]};
            const double n1 = h1[0] * h1[0] + h1[1] * h1[1] + h1[2] * h1[2], n2 = h2[0] * h2[0] + h2[1] * h2[1] + h2[2] * h2[2];
            const double k = 1.0 / sqrt(0.5 * (n1 + n2));
#pragma unroll
            for (int i = 0; i < 3; ++i) { h1[i] *= k; h2[i] *= k; }
            double v[5], a[5], b[5];
            intr_constraint(h1, h2, v);
            intr_constraint(h1, h1, a);
            intr_constraint(h2, h2, b);
#pragma unroll
            for (int i = 0; i < 5; ++i) a[i] = 0.5 * (a[i] - b[i]);
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int q = 0; q <= i; ++q) M[pnp_tri(i, q)] = fma(v[i], v[q], fma(a[i], a[q], M[pnp_tri(i, q)]));
        }
#pragma unroll
        for (int k = 0; k < 15; ++k) M[k] = group_sum<G>(M[k]);
        // eigenvalues of V'V: the conditioning diagnostic whatever the model
        double A[5][5], V[5][5];
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int q = 0; q < 5; ++q) A[i][q] = i >= q ? M[pnp_tri(i, q)] : M[pnp_tri(q, i)];
        pnp_jacobi<5>(A, V, INTR_JACOBI_SWEEPS);
        double l_min = A[0][0], l_max = A[0][0], b[5] = {V[0][0], V[1][0], V[2][0], V[3][0], V[4][0]};
        int i_min = 0;
#pragma unroll
        for (int i = 1; i < 5; ++i) {
            l_max = fmax(l_max, A[i][i]);
            if (A[i][i] < l_min) {
                l_min = A[i][i];
                i_min = i;
#pragma unroll
                for (int k = 0; k < 5; ++k) b[k] = V[k][i];
            }
        }
        double l_2nd = INFINITY;
#pragma unroll
        for (int i = 0; i < 5; ++i)
            if (i != i_min) l_2nd = fmin(l_2nd, A[i][i]);
        ratio = l_min / l_2nd;
        bool full_ok = false;
        if (model == INTR_MODEL_FULL && n_used >= 2 && l_2nd > INTR_RANK_TOL * l_max) {
            const double B11 = b[0], B22 = b[1], B13 = b[2], B23 = b[3], B33 = b[4];
            const double lam = B33 - B13 * B13 / B11 - B23 * B23 / B22;
            if (B11 * B22 > 0.0 && lam / B11 > 0.0) {
                out[0] = sqrt(lam / B11) * sc; out[1] = -B13 / B11 * sc + c0x;
                out[2] = sqrt(lam / B22) * sc; out[3] = -B23 / B22 * sc + c0y;
                full_ok = isfinite(out[0]) && isfinite(out[1]) && isfinite(out[2]) && isfinite(out[3]);
            }
        }
        if (full_ok) {
            status = INTR_FULL;
        } else {   // [[M00 M01] [M01 M11]] (1/fx^2, 1/fy^2)' = -(M04, M14)'
            const double m00 = M[pnp_tri(0, 0)], m01 = M[pnp_tri(1, 0)], m11 = M[pnp_tri(1, 1)], r0 = -M[pnp_tri(4, 0)], r1 = -M[pnp_tri(4, 1)];
            const double det = m00 * m11 - m01 * m01;
            const double ia = (r0 * m11 - r1 * m01) / det, ib = (r1 * m00 - r0 * m01) / det;
            const bool ok = det > INTR_RANK_TOL * (m00 * m11) && ia > 0.0 && ib > 0.0 && ia < INFINITY && ib < INFINITY;
            out[0] = ok ? sc / sqrt(ia) : __builtin_nan(""); out[1] = ok ? c0x : __builtin_nan("");
            out[2] = ok ? sc / sqrt(ib) : __builtin_nan(""); out[3] = ok ? c0y : __builtin_nan("");
            const bool fin = ok && isfinite(out[0]) && isfinite(out[1]) && isfinite(out[2]) && isfinite(out[3]);
            if (!fin) out[0] = out[1] = out[2] = out[3] = __builtin_nan("");
            status = !fin ? INTR_NOT_ESTIMATED : (model == INTR_MODEL_FULL ? INTR_FOCAL_FALLBACK : INTR_FOCAL);
        }
    }
    if (g == 0) {
        const bool est = status != INTR_NOT_ESTIMATED;
#pragma unroll
        for (int k = 0; k < 4; ++k) intr_out[9 * cam + k] = out[k];
#pragma unroll
        for (int k = 4; k < 9; ++k) intr_out[9 * cam + k] = est ? 0.0 : __builtin_nan("");
        info_out[2 * cam + 0] = status;
        info_out[2 * cam + 1] = n_used;
        eig_out[cam] = ratio;
    }
}

}  // namespace pcs
