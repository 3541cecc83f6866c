// ba_pnp.hpp — batched target-pose estimation (PnP) per (camera, image) view.
//
// The first step of the reference's calc_initial_params: AbstractTarget.target_pose_in_cam_image (calibration_targets/abstract_target.py:345-405)
// hands a view's detections of the known target and the camera's intrinsics to cv2.solvePnPGeneric and keeps the solution of lowest
// error; estimate_camera_relative_poses (optimisation/template_handler.py:468-601) does so for every camera and image.  Here every view is
// one group of G lanes; what such a group guarantees is in DESIGN.md, "Batched handles".  Two kernels, so that the registers of the
// 11 x 11 start do not set the occupancy of the LM passes:
//
// pnp_start_kernel — the linear start, no prior needed (after OpenCV's iterative PnP):
//   (a) measurements to normalised image coordinates with the triangulation's five fixed-point steps (undistort5_fast);
//   (b) centroid c and scatter S of the view's template points (two passes), eigen-decomposition of S (cyclic Jacobi), scale
//       s = sqrt(tr S / n); planar when lambda_min < 1e-3 lambda_mid (OpenCV's rule);
//       planar: points in the plane's frame (e1, e2, e3 = normal), q = (e1, e2)' (X - c) / s; homography with h33 = 1 by the 8 x 8 normal
//         equations (LDL'); M = [h1, h2, h1 x h2 / m] / m with m = sqrt((|h1|^2 + |h2|^2) / 2), R' = nearest rotation of M, t' = (s / m) h3;
//         R = R' [e1 e2 e3]', t = t' - R c.  The second pose of the planar ambiguity mirrors the tilt about the line of sight v = t' / |t'|
//         with the target's centre kept in place: R2 = (2 v v' - I) R (2 e3 e3' - I), t2 = t' - R2 c;
//       otherwise: q = (X - c) / s, 3 x 4 DLT with p34 = 1 by the 11 x 11 normal equations; R = nearest rotation of the left block M
//         (det M > 0 required), t' = (s / mean singular value of M) p4, t = t' - R c.
//       Both fits are one routine (pnp_fit<D>, D = 2 or 3; the measurement's image point comes from a functor, here PnpCameraMap): unknowns [row 0 (D + 1) | row 1 (D + 1) | row 2 (D)], normal matrix
//       [[A 0 B1] [0 A B2] [B1' B2' C]].  Fixing the last element to 1 is sound because t_z > 0 for a target in front of the camera.
//       Nearest rotation: M (M'M)^(-1/2) from the Jacobi eigenvectors of M'M.  The result does not depend on the choice of the in-plane
//       eigenvectors (a square grid has lambda_1 = lambda_2): the fit and every later step are covariant under it.
// pnp_lm_kernel — (c) Levenberg-Marquardt on the MEASURED pixels, full Brown-Conrady model, from the start and (planar views, when
//   at least one trial is allowed) from the second pose; the lower final cost is kept — the reference's argmin over solvePnPGeneric's
//   solutions.  Parameters (d omega, d t) of R <- exp([d omega]x) R, t <- t + d t: d X_cam = -[R X]x d omega + d t.  One pass per trial
//   accumulates 21 + 6 + 2 sums (H = J'J, g = J'r, cost, points with depth <= 0 or non-finite).  Damping, accept and stop rules:
//   DESIGN.md; xtol measures the step against the Frobenius size of [R | t].  The first V observations of a lane (measurement, key,
//   template point) stay in registers, further ones are re-read in every pass (L2-resident).
//   A pose that no accepted trial moved is returned with the bits of its start.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_device.hpp"
#include "ba_triangulate.hpp"

namespace pcs {

// status codes (include/pcs_hip.h PCS_PNP_*)
constexpr int PNP_NOT_ESTIMATED = 0;   // fewer than min_points observations, a non-finite start or a start behind the camera: NaN pose
constexpr int PNP_CONVERGED = 1;       // ftol, xtol or gtol
constexpr int PNP_MAX_ITER = 2;        // max_iter trials used
constexpr int PNP_NO_DECREASE = 3;     // the damping grew past its limit, or the damped system lost definiteness
constexpr double PNP_LAMBDA0 = 1e-4, PNP_LAMBDA_MAX = 1e10, PNP_LAMBDA_MIN = 1e-15;
constexpr double PNP_PLANAR_RATIO = 1e-3;

__device__ __forceinline__ constexpr int pnp_tri(const int i, const int j) { return i * (i + 1) / 2 + j; }   // packed lower triangle, i >= j

// exp([r]x), row-major, from the half angle: sin th = 2 s c, 1 - cos th = 2 s^2 (no cancellation at small angles)
__device__ __forceinline__ void pnp_rodrigues(const double (&r)[3], double (&R)[9]) {
    const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    double A, B;
    if (th2 < 1e-16) {
        A = 1.0 - th2 / 6.0;
        B = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        double s, c;
        sincos(0.5 * th, &s, &c);
        A = 2.0 * s * c / th;
        B = 2.0 * s * s / th2;
    }
    R[0] = 1.0 + B * (r[0] * r[0] - th2); R[1] = -A * r[2] + B * r[0] * r[1];   R[2] = A * r[1] + B * r[0] * r[2];
    R[3] = A * r[2] + B * r[1] * r[0];    R[4] = 1.0 + B * (r[1] * r[1] - th2); R[5] = -A * r[0] + B * r[1] * r[2];
    R[6] = -A * r[1] + B * r[2] * r[0];   R[7] = A * r[0] + B * r[2] * r[1];    R[8] = 1.0 + B * (r[2] * r[2] - th2);
}

// rotation matrix -> Rodrigues vector with |r| <= pi through the quaternion (largest-pivot branch): finite at angle pi
__device__ __forceinline__ void pnp_rotvec(const double (&R)[9], double (&r)[3]) {
    const double tr = R[0] + R[4] + R[8];
    double w, x, y, z;
    if (tr > 0.0) {
        const double S = 2.0 * sqrt(tr + 1.0);
        w = 0.25 * S; x = (R[7] - R[5]) / S; y = (R[2] - R[6]) / S; z = (R[3] - R[1]) / S;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double S = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        w = (R[7] - R[5]) / S; x = 0.25 * S; y = (R[1] + R[3]) / S; z = (R[2] + R[6]) / S;
    } else if (R[4] >= R[8]) {
        const double S = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        w = (R[2] - R[6]) / S; x = (R[1] + R[3]) / S; y = 0.25 * S; z = (R[5] + R[7]) / S;
    } else {
        const double S = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        w = (R[3] - R[1]) / S; x = (R[2] + R[6]) / S; y = (R[5] + R[7]) / S; z = 0.25 * S;
    }
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double n = sqrt(x * x + y * y + z * z);
    const double k = n > 1e-150 ? 2.0 * atan2(n, w) / n : 2.0;
    r[0] = k * x; r[1] = k * y; r[2] = k * z;
}

// one Jacobi rotation of the symmetric N x N matrix A (full storage) in the (P, Q) plane; V accumulates the eigenvectors in its columns
template <int N, int P, int Q>
__device__ __forceinline__ void pnp_jacobi_rotate(double (&A)[N][N], double (&V)[N][N]) {
    const double apq = A[P][Q];
    if (apq == 0.0 || !isfinite(apq)) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (!isfinite(theta)) t = 0.0;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < N; ++r) {
        if (r == P || r == Q) continue;
        const double arp = A[r][P], arq = A[r][Q];
        A[r][P] = A[P][r] = c * arp - s * arq;
        A[r][Q] = A[Q][r] = s * arp + c * arq;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double vp = V[k][P], vq = V[k][Q];
        V[k][P] = c * vp - s * vq;
        V[k][Q] = s * vp + c * vq;
    }
}

// one cyclic sweep: the pairs (0, 1), (0, 2), ..., (N - 2, N - 1), every index a compile-time constant (the matrices stay in registers)
template <int N, int P = 0, int Q = 1>
__device__ __forceinline__ void pnp_jacobi_sweep(double (&A)[N][N], double (&V)[N][N]) {
    pnp_jacobi_rotate<N, P, Q>(A, V);
    if constexpr (Q + 1 < N) pnp_jacobi_sweep<N, P, Q + 1>(A, V);
    else if constexpr (P + 2 < N) pnp_jacobi_sweep<N, P + 1, P + 2>(A, V);
}

// eigenvalues (the diagonal of A on return, unsorted) and eigenvectors (columns of V) of a symmetric N x N by cyclic Jacobi sweeps
template <int N>
__device__ __forceinline__ void pnp_jacobi(double (&A)[N][N], double (&V)[N][N], const int sweeps) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < sweeps; ++sweep) pnp_jacobi_sweep<N>(A, V);
}

// the symmetric 3 x 3 case: eight sweeps
__device__ __forceinline__ void pnp_jacobi3(double (&A)[3][3], double (&V)[3][3]) { pnp_jacobi<3>(A, V, 8); }

// nearest rotation of M (row-major): the polar factor M (M'M)^(-1/2); sig = mean singular value
__device__ __forceinline__ void pnp_nearest_rotation(const double (&M)[9], double (&R)[9], double &sig) {
    double A[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i][j] = M[i] * M[j] + M[3 + i] * M[3 + j] + M[6 + i] * M[6 + j];
    pnp_jacobi3(A, V);
    const double s0 = sqrt(A[0][0]), s1 = sqrt(A[1][1]), s2 = sqrt(A[2][2]);
    sig = (s0 + s1 + s2) / 3.0;
    const double i0 = 1.0 / s0, i1 = 1.0 / s1, i2 = 1.0 / s2;
    double W[3][3];   // V diag(1 / sig) V'
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) W[i][j] = V[i][0] * i0 * V[j][0] + V[i][1] * i1 * V[j][1] + V[i][2] * i2 * V[j][2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = M[3 * i] * W[0][j] + M[3 * i + 1] * W[1][j] + M[3 * i + 2] * W[2][j];
}

// A x = b by LDL' without pivoting on the packed lower triangle (destroyed); false when a pivot is not positive and finite or x is not finite
template <int N>
__device__ __forceinline__ bool pnp_ldl(double (&A)[N * (N + 1) / 2], const double (&b)[N], double (&x)[N]) {
    bool ok = true;
    double inv[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = A[pnp_tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= A[pnp_tri(j, k)] * A[pnp_tri(j, k)] * A[pnp_tri(k, k)];
        A[pnp_tri(j, j)] = d;
        ok = ok && d > 0.0 && d < INFINITY;
        inv[j] = tri_rcp(d);
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            double l = A[pnp_tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) l -= A[pnp_tri(i, k)] * A[pnp_tri(j, k)] * A[pnp_tri(k, k)];
            A[pnp_tri(i, j)] = l * inv[j];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {   // L y = b
        double y = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) y -= A[pnp_tri(i, k)] * x[k];
        x[i] = y;
    }
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {   // L' x = y / D
        double y = x[i] * inv[i];
#pragma unroll
        for (int k = i + 1; k < N; ++k) y -= A[pnp_tri(k, i)] * x[k];
        x[i] = y;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) ok = ok && isfinite(x[i]);
    return ok;
}

// measurement -> normalised image point of the PnP start: the camera table's five fixed-point undistortion steps, then the pinhole inverse
struct PnpCameraMap {
    const double *ct;
    double cx, cy, ifx, ify;
    __device__ __forceinline__ explicit PnpCameraMap(const double *__restrict__ t) : ct(t), cx(t[23]), cy(t[25]), ifx(tri_rcp(t[22])), ify(tri_rcp(t[24])) {}
    __device__ __forceinline__ void operator()(const double2 m, double &x, double &y) const {
        double uo, vo;
        undistort5_fast(m.x, m.y, ct, uo, vo);
        x = (uo - cx) * ifx;
        y = (vo - cy) * ify;
    }
};

// Least squares of the projective map with its last element 1 from q = F (X - c) inv_s (D coordinates) to the image point that
// `to_image` makes of a measurement (PnpCameraMap; ba_intrinsics.hpp: Hartley-normalised pixels): the group's normal equations (every
// lane identical bits) and their solution h (3 D + 2).
template <int D, int G, class Map>
__device__ __forceinline__ bool pnp_fit(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t s0, const int64_t s1, const int g,
                                        const Map &to_image, const double *__restrict__ pts, const double (&c)[3], const double (&F)[D][3],
                                        const double inv_s, double (&h)[3 * D + 2]) {
    constexpr int M = D + 1, N = 3 * D + 2;
    double A[N * (N + 1) / 2], b[N];
#pragma unroll
    for (int k = 0; k < N * (N + 1) / 2; ++k) A[k] = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k) b[k] = 0.0;
    for (int64_t o = s0 + g; o < s1; o += G) {
        const double2 m = uv[o];
        const double *X = pts + 3 * (int64_t)key[o];
        const double d0 = X[0] - c[0], d1 = X[1] - c[1], d2 = X[2] - c[2];
        double q[D], qt[M];
#pragma unroll
        for (int k = 0; k < D; ++k) qt[k] = q[k] = (F[k][0] * d0 + F[k][1] * d1 + F[k][2] * d2) * inv_s;
        qt[D] = 1.0;
        double x, y;
        to_image(m, x, y);
        const double w = x * x + y * y;
#pragma unroll
        for (int i = 0; i < M; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) A[pnp_tri(i, j)] = fma(qt[i], qt[j], A[pnp_tri(i, j)]);
            b[i] = fma(x, qt[i], b[i]);
            b[M + i] = fma(y, qt[i], b[M + i]);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                A[pnp_tri(2 * M + i, j)] = fma(-x * q[i], qt[j], A[pnp_tri(2 * M + i, j)]);
                A[pnp_tri(2 * M + i, M + j)] = fma(-y * q[i], qt[j], A[pnp_tri(2 * M + i, M + j)]);
            }
#pragma unroll
            for (int j = 0; j <= i; ++j) A[pnp_tri(2 * M + i, 2 * M + j)] = fma(w * q[i], q[j], A[pnp_tri(2 * M + i, 2 * M + j)]);
            b[2 * M + i] = fma(-w, q[i], b[2 * M + i]);
        }
    }
    if constexpr (G > 1) {
#pragma unroll
        for (int i = 0; i < M; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) A[pnp_tri(i, j)] = group_sum<G>(A[pnp_tri(i, j)]);
#pragma unroll
        for (int i = 2 * M; i < N; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) A[pnp_tri(i, j)] = group_sum<G>(A[pnp_tri(i, j)]);
#pragma unroll
        for (int k = 0; k < N; ++k) b[k] = group_sum<G>(b[k]);
    }
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) A[pnp_tri(M + i, M + j)] = A[pnp_tri(i, j)];   // the second diagonal block is the first
    return pnp_ldl<N>(A, b, h);
}

// Centroid c (two passes: centroid, then scatter) of a group's template points, the frame of their scatter (e3: the eigenvector of the
// smallest eigenvalue, the normal of a planar target; e1: of the largest; e2 = e3 x e1), the smallest and the middle eigenvalue and
// the scale s = sqrt(tr S / n).  The view is planar when l_min < PNP_PLANAR_RATIO l_mid.  Every lane of the group gets identical bits.
// (The eigenvector matrix stays local to this routine: selected through a reference it would be indexed dynamically, in scratch.)
template <int G>
__device__ __forceinline__ void pnp_template_frame(const int32_t *__restrict__ key, const double *__restrict__ pts, const int64_t s0, const int64_t s1,
                                                   const int g, const int64_t n, double (&c)[3], double (&e1)[3], double (&e2)[3], double (&e3)[3],
                                                   double &l_min, double &l_mid, double &s) {
    c[0] = c[1] = c[2] = 0.0;
    for (int64_t o = s0 + g; o < s1; o += G) {
        const double *X = pts + 3 * (int64_t)key[o];
        c[0] += X[0]; c[1] += X[1]; c[2] += X[2];
    }
    const double inv_n = 1.0 / (double)n;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = group_sum<G>(c[k]) * inv_n;
    double S[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t o = s0 + g; o < s1; o += G) {
        const double *X = pts + 3 * (int64_t)key[o];
        const double d0 = X[0] - c[0], d1 = X[1] - c[1], d2 = X[2] - c[2];
        S[0] = fma(d0, d0, S[0]); S[1] = fma(d0, d1, S[1]); S[2] = fma(d0, d2, S[2]);
        S[3] = fma(d1, d1, S[3]); S[4] = fma(d1, d2, S[4]); S[5] = fma(d2, d2, S[5]);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) S[k] = group_sum<G>(S[k]);
    double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}}, E[3][3];
    pnp_jacobi3(A, E);
    const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
    // three distinct indices: the first minimum, then the first maximum of the other two.  Equal eigenvalues (an isotropic target,
    // such as the corners of a cube) are simply not planar.
    const int i_min = (l0 <= l1 && l0 <= l2) ? 0 : (l1 <= l2 ? 1 : 2);
    const int o_a = i_min == 0 ? 1 : 0, o_b = i_min == 2 ? 1 : 2;
    const double l_a = o_a == 0 ? l0 : l1, l_b = o_b == 1 ? l1 : l2;
    const int i_max = l_a >= l_b ? o_a : o_b;
    s = sqrt((l0 + l1 + l2) * inv_n);
    l_min = i_min == 0 ? l0 : (i_min == 1 ? l1 : l2);
    l_mid = l_a >= l_b ? l_b : l_a;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e3[k] = i_min == 0 ? E[k][0] : (i_min == 1 ? E[k][1] : E[k][2]);
        e1[k] = i_max == 0 ? E[k][0] : (i_max == 1 ? E[k][1] : E[k][2]);
    }
    e2[0] = e3[1] * e1[2] - e3[2] * e1[1]; e2[1] = e3[2] * e1[0] - e3[0] * e1[2]; e2[2] = e3[0] * e1[1] - e3[1] * e1[0];
}

__device__ __forceinline__ void pnp_write_nan(double *__restrict__ p) {
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = __builtin_nan("");
}

template <int G>
__global__ __launch_bounds__(256) void pnp_start_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                        const int32_t *__restrict__ view_cam, const double *__restrict__ cam_tab,
                                                        const double *__restrict__ pts, const int64_t n_views, const int32_t *__restrict__ order,
                                                        const int min_points, double *__restrict__ pose_init, double *__restrict__ pose_alt) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_views) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t j = order ? order[gid] : gid;
    const int64_t s0 = start[j], s1 = start[j + 1];
    const int64_t n = s1 - s0;
    double *po = pose_init + 6 * j, *pa = pose_alt + 6 * j;
    if (n <= 0 || n < min_points) {
        if (g == 0) { pnp_write_nan(po); pnp_write_nan(pa); }
        return;
    }
    const double *ct = cam_tab + (int64_t)view_cam[j] * TRI_CAM_STRIDE;
    double c[3], e1[3], e2[3], e3[3], l_min, l_mid, s;
    pnp_template_frame<G>(key, pts, s0, s1, g, n, c, e1, e2, e3, l_min, l_mid, s);
    bool ok = true;
    double pose[6], alt[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pose[k] = alt[k] = __builtin_nan("");
    const double inv_s = 1.0 / s;
    if (ok && l_min < PNP_PLANAR_RATIO * l_mid) {   // planar
        const double F[2][3] = {{e1[0], e1[1], e1[2]}, {e2[0], e2[1], e2[2]}};
        double h[8];
        ok = pnp_fit<2, G>(key, uv, s0, s1, g, PnpCameraMap(ct), pts, c, F, inv_s, h);
        if (ok) {
            const double c1[3] = {h[0], h[3], h[6]}, c2[3] = {h[1], h[4], h[7]}, c3[3] = {h[2], h[5], 1.0};
            const double nrm = sqrt(0.5 * (c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2] + c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]));
            const double in = 1.0 / nrm;
            const double x3[3] = {c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0]};
            double M[9], Rp[9], sig;
#pragma unroll
            for (int r = 0; r < 3; ++r) { M[3 * r] = c1[r] * in; M[3 * r + 1] = c2[r] * in; M[3 * r + 2] = x3[r] * in * in; }
            pnp_nearest_rotation(M, Rp, sig);
            const double tp[3] = {s * in * c3[0], s * in * c3[1], s * in * c3[2]};
            double R[9], T[9], R2[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k) R[3 * r + k] = Rp[3 * r] * e1[k] + Rp[3 * r + 1] * e2[k] + Rp[3 * r + 2] * e3[k];
            const double itn = 1.0 / sqrt(tp[0] * tp[0] + tp[1] * tp[1] + tp[2] * tp[2]);
            const double v[3] = {tp[0] * itn, tp[1] * itn, tp[2] * itn};
#pragma unroll
            for (int r = 0; r < 3; ++r) {   // T = R (2 e3 e3' - I)
                const double re = R[3 * r] * e3[0] + R[3 * r + 1] * e3[1] + R[3 * r + 2] * e3[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) T[3 * r + k] = 2.0 * re * e3[k] - R[3 * r + k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {   // R2 = (2 v v' - I) T
                const double vt = v[0] * T[k] + v[1] * T[3 + k] + v[2] * T[6 + k];
#pragma unroll
                for (int r = 0; r < 3; ++r) R2[3 * r + k] = 2.0 * v[r] * vt - T[3 * r + k];
            }
            double rv[3], rv2[3];
            pnp_rotvec(R, rv);
            pnp_rotvec(R2, rv2);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                pose[r] = rv[r];
                alt[r] = rv2[r];
                pose[3 + r] = tp[r] - (R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]);
                alt[3 + r] = tp[r] - (R2[3 * r] * c[0] + R2[3 * r + 1] * c[1] + R2[3 * r + 2] * c[2]);
            }
        }
    } else if (ok) {   // a 3-D view
        const double F[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        double p[11];
        ok = pnp_fit<3, G>(key, uv, s0, s1, g, PnpCameraMap(ct), pts, c, F, inv_s, p);
        const double M[9] = {p[0], p[1], p[2], p[4], p[5], p[6], p[8], p[9], p[10]};
        const double det = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
        ok = ok && det > 0.0;
        if (ok) {
            double R[9], sig, rv[3];
            pnp_nearest_rotation(M, R, sig);
            const double k = s / sig;
            const double tp[3] = {k * p[3], k * p[7], k};
            pnp_rotvec(R, rv);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                pose[r] = rv[r];
                pose[3 + r] = tp[r] - (R[3 * r] * c[0] + R[3 * r + 1] * c[1] + R[3 * r + 2] * c[2]);
            }
        }
    }
    bool fin = ok, fin2 = ok;
#pragma unroll
    for (int k = 0; k < 6; ++k) { fin = fin && isfinite(pose[k]); fin2 = fin2 && isfinite(alt[k]); }
    if (g == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            po[k] = fin ? pose[k] : __builtin_nan("");
            pa[k] = fin && fin2 ? alt[k] : __builtin_nan("");
        }
    }
}

// s: H (21, packed upper by rows: 00 01 .. 05 11 .. 55) | g (6) | cost | bad points
constexpr int PNP_SUMS = 29;

// one observation at the pose (R, t): residual, Jacobian rows, sums
__device__ __forceinline__ void pnp_point(const double (&R)[9], const double (&t)[3], const double (&cam)[9], const double X0, const double X1,
                                          const double X2, const double mu, const double mv, double &ru, double &rv, double (&Ju)[6], double (&Jv)[6],
                                          bool &front) {
    const double Y0 = fma(R[0], X0, fma(R[1], X1, R[2] * X2)), Y1 = fma(R[3], X0, fma(R[4], X1, R[5] * X2)), Y2 = fma(R[6], X0, fma(R[7], X1, R[8] * X2));
    const double Z0 = Y0 + t[0], Z1 = Y1 + t[1], Z2 = Y2 + t[2];
    front = Z2 > 0.0;
    const double iz = tri_rcp(Z2);
    const double x = Z0 * iz, y = Z1 * iz;
    const double fx = cam[0], cx = cam[1], fy = cam[2], cy = cam[3], k0 = cam[4], k1 = cam[5], p0 = cam[6], p1 = cam[7], k2 = cam[8];
    const double r2 = x * x + y * y;
    const double kup = 1.0 + k0 * r2 + k1 * (r2 * r2) + k2 * (r2 * r2 * r2);
    const double kd = k0 + 2.0 * k1 * r2 + 3.0 * k2 * (r2 * r2);
    const double xD = x * kup + 2.0 * p0 * x * y + p1 * (r2 + 2.0 * (x * x));
    const double yD = y * kup + p0 * (r2 + 2.0 * (y * y)) + 2.0 * p1 * x * y;
    ru = mu - (xD * fx + cx);
    rv = mv - (yD * fy + cy);
    const double cross = 2.0 * x * y * kd + 2.0 * p0 * x + 2.0 * p1 * y;
    const double dxx = kup + 2.0 * x * x * kd + 2.0 * p0 * y + 6.0 * p1 * x;
    const double dyy = kup + 2.0 * y * y * kd + 6.0 * p0 * y + 2.0 * p1 * x;
    const double ux = fx * dxx, uy = fx * cross, vx = fy * cross, vy = fy * dyy;
    // d pixel / d X_cam
    const double a0 = ux * iz, a1 = uy * iz, a2 = -(ux * x + uy * y) * iz;
    const double b0 = vx * iz, b1 = vy * iz, b2 = -(vx * x + vy * y) * iz;
    // a . (-[Y]x e_j) = (Y x a)_j with Y = R X
    Ju[0] = Y1 * a2 - Y2 * a1; Ju[1] = Y2 * a0 - Y0 * a2; Ju[2] = Y0 * a1 - Y1 * a0; Ju[3] = a0; Ju[4] = a1; Ju[5] = a2;
    Jv[0] = Y1 * b2 - Y2 * b1; Jv[1] = Y2 * b0 - Y0 * b2; Jv[2] = Y0 * b1 - Y1 * b0; Jv[3] = b0; Jv[4] = b1; Jv[5] = b2;
}

__device__ __forceinline__ void pnp_accumulate(double (&s)[PNP_SUMS], const double ru, const double rv, const double (&Ju)[6], const double (&Jv)[6],
                                               const bool front) {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) s[k] = fma(Ju[i], Ju[j], fma(Jv[i], Jv[j], s[k]));
#pragma unroll
    for (int i = 0; i < 6; ++i) s[21 + i] = fma(Ju[i], ru, fma(Jv[i], rv, s[21 + i]));
    s[27] = fma(ru, ru, fma(rv, rv, s[27]));
    s[28] += front ? 0.0 : 1.0;   // behind the camera (NaN depths are not > 0 either)
}

// The robust twin of pnp_accumulate (the robust rigpose_lm_kernel; pnp_lm_kernel takes no loss): u and v are scaled separately by
// robust_rho — row s J, residual rho1 f / s — so that s[0..21) = sum s^2 J'J, s[21..27) = sum J' rho1 f and s[27] = sum rho0, the cost
// the loop watches.  `raw` takes the plain sum of squares, which the reported RMS needs.
__device__ __forceinline__ void pnp_accumulate_robust(double (&s)[PNP_SUMS], double &raw, const GroupLoss &loss, const double ru, const double rv,
                                                      const double (&Ju)[6], const double (&Jv)[6], const bool front) {
    double q0, q1, fu, fv, Su[6], Sv[6];
    const double su = robust_rho(loss.kind, ru, loss.inv_f_scale, loss.f_scale_sq, q0, fu);
    const double sv = robust_rho(loss.kind, rv, loss.inv_f_scale, loss.f_scale_sq, q1, fv);
#pragma unroll
    for (int i = 0; i < 6; ++i) Su[i] = su * Ju[i], Sv[i] = sv * Jv[i];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) s[k] = fma(Su[i], Su[j], fma(Sv[i], Sv[j], s[k]));
#pragma unroll
    for (int i = 0; i < 6; ++i) s[21 + i] = fma(Su[i], fu, fma(Sv[i], fv, s[21 + i]));
    s[27] += q0 + q1;
    s[28] += front ? 0.0 : 1.0;
    raw = fma(ru, ru, fma(rv, rv, raw));
}

// (H + lam diag(H)) d = g; false when the damped system is not positive definite or d is not finite
__device__ __forceinline__ bool pnp_solve(const double (&s)[PNP_SUMS], const double lam, double (&d)[6]) {
    double A[21], b[6];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++k) A[pnp_tri(j, i)] = i == j ? s[k] * (1.0 + lam) : s[k];
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = s[21 + i];
    return pnp_ldl<6>(A, b, d);
}

template <int G, int V>
__global__ __launch_bounds__(256) void pnp_lm_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                     const int32_t *__restrict__ view_cam, const double *__restrict__ cam_tab,
                                                     const double *__restrict__ pts, const int64_t n_views, const int32_t *__restrict__ order,
                                                     const double *__restrict__ pose_init, const double *__restrict__ pose_alt, const int max_iter,
                                                     const double ftol, const double xtol, const double gtol, const int min_points,
                                                     double *__restrict__ pose_out, double *__restrict__ rms_out, int32_t *__restrict__ info_out,
                                                     double *__restrict__ resid_out) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    const bool live = gid < n_views;   // whole groups are live or dead; a dead group never takes part in a pass
    const int64_t jv = live ? gid : n_views - 1;
    const int64_t j = order ? order[jv] : jv;
    const int64_t s0 = start[j], s1 = live ? start[j + 1] : s0;
    const int64_t n = s1 - s0;
    const bool enough = live && n > 0 && n >= min_points;
    int nv = enough ? (int)((n - g + G - 1) / G) : 0;
    nv = nv < 0 ? 0 : (nv > V ? V : nv);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nv = max(nv, __shfl_xor(nv, off));
    const int nv_w = __builtin_amdgcn_readfirstlane(nv);   // the wave's largest number of register observations per lane (uniform)

    double2 m[V];
    double Xr[V][3];
    bool have[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        m[v] = make_double2(0.0, 0.0);
        Xr[v][0] = Xr[v][1] = Xr[v][2] = 0.0;
        have[v] = false;
        if (v >= nv_w) continue;
        const int64_t q = s0 + g + (int64_t)v * G;
        if (enough && q < s1) {
            m[v] = uv[q];
            const double *X = pts + 3 * (int64_t)key[q];
            Xr[v][0] = X[0]; Xr[v][1] = X[1]; Xr[v][2] = X[2];
            have[v] = true;
        }
    }
    double cam[9];
    {
        const double *ct = cam_tab + (int64_t)view_cam[j] * TRI_CAM_STRIDE + 22;
#pragma unroll
        for (int k = 0; k < 9; ++k) cam[k] = ct[k];
    }
    // one pass: the group's sums at (R, t) (every lane of the group gets identical bits)
    auto pass = [&](const double (&R)[9], const double (&t)[3], double (&s)[PNP_SUMS]) {
#pragma unroll
        for (int k = 0; k < PNP_SUMS; ++k) s[k] = 0.0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            if (v >= nv_w) break;
            if (have[v]) {
                double ru, rv, Ju[6], Jv[6];
                bool front;
                pnp_point(R, t, cam, Xr[v][0], Xr[v][1], Xr[v][2], m[v].x, m[v].y, ru, rv, Ju, Jv, front);
                pnp_accumulate(s, ru, rv, Ju, Jv, front);
            }
        }
        for (int64_t q = s0 + g + (int64_t)V * G; q < s1; q += G) {   // observations beyond the registers
            const double2 mq = uv[q];
            const double *X = pts + 3 * (int64_t)key[q];
            double ru, rv, Ju[6], Jv[6];
            bool front;
            pnp_point(R, t, cam, X[0], X[1], X[2], mq.x, mq.y, ru, rv, Ju, Jv, front);
            pnp_accumulate(s, ru, rv, Ju, Jv, front);
        }
        if constexpr (G > 1) {
#pragma unroll
            for (int k = 0; k < PNP_SUMS; ++k) s[k] = group_sum<G>(s[k]);
        }
    };

    double best[6], best_cost = 0.0, cost_init = 0.0;
    int best_it = 0, best_status = PNP_NOT_ESTIMATED;
#pragma unroll
    for (int k = 0; k < 6; ++k) best[k] = __builtin_nan("");
#pragma unroll 1
    for (int cand = 0; cand < 2; ++cand) {
        // candidate 0: the start; candidate 1: the second pose of a planar view, tried when trials are allowed and the start was usable
        const double *p0 = (cand == 0 ? pose_init : pose_alt) + 6 * j;
        double ps[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) ps[k] = p0[k];
        bool fin = enough && (cand == 0 || (max_iter > 0 && best_status != PNP_NOT_ESTIMATED));
#pragma unroll
        for (int k = 0; k < 6; ++k) fin = fin && isfinite(ps[k]);
        double R[9], t[3] = {ps[3], ps[4], ps[5]}, cur[PNP_SUMS], cost0 = 0.0;
        {
            const double r[3] = {ps[0], ps[1], ps[2]};
            pnp_rodrigues(r, R);
        }
        int status = PNP_NOT_ESTIMATED, it = 0;
        bool done = true, moved = false;
        if (fin) {   // cost, H and g at the start
            pass(R, t, cur);
            cost0 = cur[27];
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
                pass(Rt, tt, s);
                ++it;
                const double step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
                const double size = sqrt(3.0 + t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);   // Frobenius size of [R | t]
                const bool small = step <= xtol * (xtol + size);
                if (s[28] == 0.0 && s[27] < cur[27]) {   // accepted: lower cost, every point in front (a NaN cost is not lower)
                    const bool flat = cur[27] - s[27] <= ftol * cur[27];
#pragma unroll
                    for (int k = 0; k < 9; ++k) R[k] = Rt[k];
                    t[0] = tt[0]; t[1] = tt[1]; t[2] = tt[2];
#pragma unroll
                    for (int k = 0; k < PNP_SUMS; ++k) cur[k] = s[k];
                    moved = true;
                    lam = fmax(lam * 0.1, PNP_LAMBDA_MIN);
                    if (flat || small) { status = PNP_CONVERGED; done = true; }
                } else {
                    lam *= 10.0;
                    if (small) { status = PNP_CONVERGED; done = true; }
                    else if (lam > PNP_LAMBDA_MAX) { status = PNP_NO_DECREASE; done = true; }
                }
            }
        }
        if (cand == 0) cost_init = cost0;
        if (usable && (cand == 0 || cur[27] < best_cost)) {
            if (moved) {
                double rv[3];
                pnp_rotvec(R, rv);
                best[0] = rv[0]; best[1] = rv[1]; best[2] = rv[2];
                best[3] = t[0]; best[4] = t[1]; best[5] = t[2];
            } else {
#pragma unroll
                for (int k = 0; k < 6; ++k) best[k] = ps[k];   // never moved: the start's bits
            }
            best_cost = cur[27];
            best_it = it;
            best_status = status;
        }
    }
    if (!live) return;
    const bool est = best_status != PNP_NOT_ESTIMATED;
    if (g == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) pose_out[6 * j + k] = best[k];
        const double inv_n = 1.0 / (double)n;
        rms_out[2 * j + 0] = est ? sqrt(best_cost * inv_n) : __builtin_nan("");
        rms_out[2 * j + 1] = est ? sqrt(cost_init * inv_n) : __builtin_nan("");
        info_out[3 * j + 0] = best_it;
        info_out[3 * j + 1] = best_status;
        info_out[3 * j + 2] = (int32_t)n;
    }
    if (resid_out) {   // residuals at the returned pose, in observation order (NaN where no pose was estimated)
        double R[9];
        const double r[3] = {best[0], best[1], best[2]}, t[3] = {best[3], best[4], best[5]};
        pnp_rodrigues(r, R);
        for (int64_t q = s0 + g; q < s1; q += G) {
            const double2 mq = uv[q];
            const double *X = pts + 3 * (int64_t)key[q];
            double ru, rv, Ju[6], Jv[6];
            bool front;
            pnp_point(R, t, cam, X[0], X[1], X[2], mq.x, mq.y, ru, rv, Ju, Jv, front);
            resid_out[2 * q + 0] = est ? ru : __builtin_nan("");
            resid_out[2 * q + 1] = est ? rv : __builtin_nan("");
        }
    }
}

}  // namespace pcs
