// ba_twoview.hpp — relative pose of two cameras from their shared image points, consensus-based (pcs_twoview_run).
//
// What cv2.findEssentialMat(..., RANSAC) + cv2.recoverPose are on the host: the one estimate of the free chain (projection + extrinsic3D
// + free_point) that needs no 3-D knowledge.  A pair p of cameras (a, b), a < b, owns rows start[p] .. start[p + 1] of a correspondence
// table (uv_a, uv_b) in measured pixels.  Policy of DESIGN.md, "Batched handles": lane g of a group owns items g, g + G, ...; group sums
// are xor-butterflies (every lane holds identical bits); no floating-point atomics; no scratch; nothing of a neighbour or of the launch
// geometry enters a result, and the hypothesis count is fixed: two runs agree bit for bit.
//
// tv_undistort_kernel    one thread per correspondence: both pixels through undistort5 (ba_triangulate.hpp) to undistorted pixels, written
//                        once and read by every later stage.
// tv_hypothesis_kernel   one group of 16 lanes per (pair, hypothesis): eight rows drawn by cons_sample_positions (ba_consensus.hpp;
//                        stream key: the pair index), the eight-point fit (tv_eight_point), the essential projection,
//                        F = K_b^-T E K_a^-1 and a usable flag.
// tv_score_kernel<G>     one group per (pair, hypothesis): sum min(e^2, tau^2) of the Sampson distance over all rows of the pair; +inf
//                        for an unusable hypothesis.
// tv_select_kernel<G>    one group per pair: the lowest score wins, ties go to the lower hypothesis; inlier flags e^2 <= tau^2, their count.
// tv_final_kernel<G>     one group per pair: the same fit over all inliers, essential projection, the four (R, +-t), cheirality, outputs.
//
// The eight-point fit.  Per image the points are shifted to their centroid and scaled to a mean squared distance of 2 (Hartley), both from
// ONE pass of sums over the pixels taken relative to the principal point; the second pass forms the 45 moment sums of the rows
// [xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1] of the epipolar constraint x_b' F x_a = 0.  The eigenvector of the smallest eigenvalue
// of the 9 x 9 moment matrix comes from a cyclic Jacobi with a fixed sweep count that keeps NO runtime-indexed array: lane r of the group
// holds row r of the matrix and row r of the eigenvector matrix in registers, the entries of a rotation (p, q) are taken by select chains,
// its angle comes from three shuffles, the column update is local to every lane and the row update of lanes p and q takes the two rows by
// shuffles.
// Denormalisation and E = K_b' F K_a are one step: N = T K = [[s fx, 0, -s mx], [0, s fy, -s my], [0, 0, 1]] maps normalised camera
// coordinates to Hartley coordinates without the principal point cancelling, E = N_b' F~ N_a.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_consensus.hpp"
#include "ba_pnp.hpp"
#include "ba_triangulate.hpp"

namespace pcs {

constexpr int TV_OK = 0;              // T = [R | t] is the pose
constexpr int TV_TOO_FEW = 1;         // fewer than max(8, min_points) correspondences
constexpr int TV_DEGENERATE = 2;      // no usable hypothesis, fewer than 8 inliers, or the fit over the inliers lost rank
constexpr int TV_NO_CHEIRALITY = 3;   // no inlier in front of both cameras for any of the four candidates
constexpr int TV_SAMPLE = 8;
constexpr int TV_SWEEPS = 10;             // cyclic Jacobi sweeps of the 9 x 9 (quadratic convergence: 6-8 reach rounding level)
constexpr double TV_RANK_RATIO = 1e-12;   // second smallest eigenvalue of the moment matrix against the largest: below, the null space is not a line

// the affine maps of the fit, all of the shape [[p, 0, u], [0, q, v], [0, 0, 1]]
struct TvAffine {
    double p, q, u, v;
};

// out = Nb' M Na (row-major 3 x 3)
__device__ __forceinline__ void tv_sandwich(const TvAffine &nb, const double (&M)[9], const TvAffine &na, double (&out)[9]) {
    double g[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[3 * i + 0] = M[3 * i + 0] * na.p;
        g[3 * i + 1] = M[3 * i + 1] * na.q;
        g[3 * i + 2] = M[3 * i + 0] * na.u + M[3 * i + 1] * na.v + M[3 * i + 2];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[j] = nb.p * g[j];
        out[3 + j] = nb.q * g[3 + j];
        out[6 + j] = nb.u * g[j] + nb.v * g[3 + j] + g[6 + j];
    }
}

// the pinhole part of both cameras of a pair: [fx, cx, fy, cy] each
struct TvCams {
    double fxa, cxa, fya, cya, fxb, cxb, fyb, cyb;
    __device__ __forceinline__ TvCams(const double *__restrict__ cam_tab, const int32_t a, const int32_t b) {
        const double *ta = cam_tab + (int64_t)a * TRI_CAM_STRIDE + 22, *tb = cam_tab + (int64_t)b * TRI_CAM_STRIDE + 22;
        fxa = ta[0]; cxa = ta[1]; fya = ta[2]; cya = ta[3];
        fxb = tb[0]; cxb = tb[1]; fyb = tb[2]; cyb = tb[3];
    }
    __device__ __forceinline__ TvAffine inv_a() const { return {1.0 / fxa, 1.0 / fya, -cxa / fxa, -cya / fya}; }
    __device__ __forceinline__ TvAffine inv_b() const { return {1.0 / fxb, 1.0 / fyb, -cxb / fxb, -cyb / fyb}; }
};

// Sampson distance of a row m = (xa, ya, xb, yb) in undistorted pixels
__device__ __forceinline__ double tv_sampson(const double (&F)[9], const double4 m) {
    const double l0 = F[0] * m.x + F[1] * m.y + F[2], l1 = F[3] * m.x + F[4] * m.y + F[5], l2 = F[6] * m.x + F[7] * m.y + F[8];   // F x_a
    const double r0 = F[0] * m.z + F[3] * m.w + F[6], r1 = F[1] * m.z + F[4] * m.w + F[7];                                      // F' x_b
    const double num = m.z * l0 + m.w * l1 + l2;
    return num * num / (l0 * l0 + l1 * l1 + r0 * r0 + r1 * r1);
}

// element `i` (the same in every lane) of a row held in registers: a select chain.  The empty asm keeps the optimiser from folding the
// chain back into an indexed load, which would move the row to scratch.
__device__ __forceinline__ double tv_pick(const double (&x)[9], const int i) {
    double v = x[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) {
        v = i == k ? x[k] : v;
        asm volatile("" : "+v"(v));
    }
    return v;
}

// one Jacobi rotation of the symmetric 9 x 9 in the (p, q) plane: lane r of the group holds A[r][.] in A and V[r][.] in V.  p and q are the
// same in every lane; the 36 rotations of a sweep share this one body (unrolled over (p, q) the kernel takes minutes to compile).
template <int G>
__device__ __forceinline__ void tv_rotate(double (&A)[9], double (&V)[9], const int g, const int p, const int q) {
    const double ap = tv_pick(A, p), aq = tv_pick(A, q), vp = tv_pick(V, p), vq = tv_pick(V, q);
    const double app = __shfl(ap, p, G), aqq = __shfl(aq, q, G), apq = __shfl(aq, p, G);
    double t = 0.0, c = 1.0, s = 0.0;
    if (apq != 0.0 && isfinite(apq)) {   // the same in every lane of the group
        const double theta = (aqq - app) / (2.0 * apq);
        t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (!isfinite(theta)) t = 0.0;
        c = 1.0 / sqrt(t * t + 1.0);
        s = t * c;
    }
    // A J and V J: columns p and q of every row, local to its lane
    const double ap1 = c * ap - s * aq, aq1 = s * ap + c * aq, vp1 = c * vp - s * vq, vq1 = s * vp + c * vq;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        A[k] = k == p ? ap1 : (k == q ? aq1 : A[k]);
        V[k] = k == p ? vp1 : (k == q ? vq1 : V[k]);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {   // J' (A J): rows p and q; their entries (p, p), (q, q), (p, q) come from the closed form
        const double rp = __shfl(A[k], p, G), rq = __shfl(A[k], q, G);
        const double np = k == p ? app - t * apq : (k == q ? 0.0 : c * rp - s * rq);
        const double nq = k == q ? aqq + t * apq : (k == p ? 0.0 : s * rp + c * rq);
        A[k] = g == p ? np : (g == q ? nq : A[k]);
    }
}

template <int G>
__device__ __forceinline__ void tv_sweep(double (&A)[9], double (&V)[9], const int g) {
#pragma unroll 1
    for (int p = 0; p < 8; ++p)
#pragma unroll 1
        for (int q = p + 1; q < 9; ++q) tv_rotate<G>(A, V, g, p, q);
}

// What a fit leaves: E before and after the projection onto the essential manifold (singular values (s, s, 0), s the mean of the two
// largest), the two right singular vectors that stay and their singular values.
struct TvFit {
    double E0[9], E[9], v1[3], v2[3], s1, s2;
};

// The eight-point fit of the rows `each` hands out (each(f) calls f(m) for every row of this lane, in its fixed order).  false: not
// finite, or the moment matrix has lost rank 8 (its null space is not a line).  Every lane of the group returns identical bits.
template <int G, class Each>
__device__ __forceinline__ bool tv_eight_point(const Each &each, const int g, const TvCams &k, TvFit &fit) {
    // pass 1: count, centroid and mean squared distance per image, pixels relative to the principal point
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    each([&](const double4 m) {
        const double xa = m.x - k.cxa, ya = m.y - k.cya, xb = m.z - k.cxb, yb = m.w - k.cyb;
        s[0] += 1.0;
        s[1] += xa; s[2] += ya; s[3] += xa * xa + ya * ya;
        s[4] += xb; s[5] += yb; s[6] += xb * xb + yb * yb;
    });
#pragma unroll
    for (int i = 0; i < 7; ++i) s[i] = group_sum<G>(s[i]);
    const double inv_n = 1.0 / s[0];
    const double mxa = s[1] * inv_n, mya = s[2] * inv_n, mxb = s[4] * inv_n, myb = s[5] * inv_n;
    const double sa = sqrt(2.0 / (s[3] * inv_n - (mxa * mxa + mya * mya))), sb = sqrt(2.0 / (s[6] * inv_n - (mxb * mxb + myb * myb)));
    // pass 2: the 45 moments of the constraint rows in Hartley coordinates
    double M[45];
#pragma unroll
    for (int i = 0; i < 45; ++i) M[i] = 0.0;
    each([&](const double4 m) {
        const double xa = sa * ((m.x - k.cxa) - mxa), ya = sa * ((m.y - k.cya) - mya), xb = sb * ((m.z - k.cxb) - mxb), yb = sb * ((m.w - k.cyb) - myb);
        const double r[9] = {xb * xa, xb * ya, xb, yb * xa, yb * ya, yb, xa, ya, 1.0};
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) M[pnp_tri(i, j)] += r[i] * r[j];
    });
#pragma unroll
    for (int i = 0; i < 45; ++i) M[i] = group_sum<G>(M[i]);
    // lane r takes row r (lanes 9 .. G - 1 hold zeros and are never a source)
    double A[9], V[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        A[c] = 0.0;
        V[c] = g == c ? 1.0 : 0.0;
#pragma unroll
        for (int r = 0; r < 9; ++r)
            if (g == r) A[c] = M[r >= c ? pnp_tri(r, c) : pnp_tri(c, r)];
    }
#pragma unroll 1
    for (int sweep = 0; sweep < TV_SWEEPS; ++sweep) tv_sweep<G>(A, V, g);
    double d[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) d[c] = __shfl(A[c], c, G);
    int jmin = 0;
    double dmin = d[0], dmax = d[0];
#pragma unroll
    for (int c = 1; c < 9; ++c) {
        if (d[c] < dmin) { dmin = d[c]; jmin = c; }
        dmax = d[c] > dmax ? d[c] : dmax;
    }
    double dsec = INFINITY;
#pragma unroll
    for (int c = 0; c < 9; ++c)
        if (c != jmin && d[c] < dsec) dsec = d[c];
    double vsel = 0.0;
#pragma unroll
    for (int c = 0; c < 9; ++c)
        if (c == jmin) vsel = V[c];
    double f[9];
    bool ok = dmax > 0.0 && dsec > TV_RANK_RATIO * dmax;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        f[c] = __shfl(vsel, c, G);
        ok = ok && isfinite(f[c]);
    }
    // E = N_b' F~ N_a
    const TvAffine na{sa * k.fxa, sa * k.fya, -sa * mxa, -sa * mya}, nb{sb * k.fxb, sb * k.fyb, -sb * mxb, -sb * myb};
    tv_sandwich(nb, f, na, fit.E0);
    // projection: E' = E (w1 v1 v1' + w2 v2 v2'), w = s / sigma, over the two largest singular values of E
    double B[3][3], W3[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i][j] = fit.E0[i] * fit.E0[j] + fit.E0[3 + i] * fit.E0[3 + j] + fit.E0[6 + i] * fit.E0[6 + j];
    pnp_jacobi3(B, W3);
    const double e0 = B[0][0], e1 = B[1][1], e2 = B[2][2];
    const int k3 = e0 <= e1 && e0 <= e2 ? 0 : (e1 <= e2 ? 1 : 2);   // the smallest: ties to the lower index
    const double sg0 = sqrt(fmax(e0, 0.0)), sg1 = sqrt(fmax(e1, 0.0)), sg2 = sqrt(fmax(e2, 0.0));
    fit.s1 = k3 == 0 ? sg1 : sg0;
    fit.s2 = k3 == 2 ? sg1 : sg2;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        fit.v1[i] = k3 == 0 ? W3[i][1] : W3[i][0];
        fit.v2[i] = k3 == 2 ? W3[i][1] : W3[i][2];
    }
    const double sm = 0.5 * (fit.s1 + fit.s2), w1 = sm / fit.s1, w2 = sm / fit.s2;
    ok = ok && fit.s1 > 0.0 && fit.s2 > 0.0;
    double Wp[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Wp[3 * i + j] = w1 * fit.v1[i] * fit.v1[j] + w2 * fit.v2[i] * fit.v2[j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            fit.E[3 * i + j] = fit.E0[3 * i] * Wp[j] + fit.E0[3 * i + 1] * Wp[3 + j] + fit.E0[3 * i + 2] * Wp[6 + j];
            ok = ok && isfinite(fit.E[3 * i + j]);
        }
    return ok;
}

__global__ __launch_bounds__(256) void tv_undistort_kernel(const double2 *__restrict__ uv_a, const double2 *__restrict__ uv_b,
                                                           const int32_t *__restrict__ corr_pair, const int32_t *__restrict__ pair_cams,
                                                           const double *__restrict__ cam_tab, const int64_t n_corr, double4 *__restrict__ und) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= n_corr) return;
    const int64_t p = corr_pair[o];
    const double2 ma = uv_a[o], mb = uv_b[o];
    double4 r;
    undistort5(ma.x, ma.y, cam_tab + (int64_t)pair_cams[2 * p] * TRI_CAM_STRIDE, r.x, r.y);
    undistort5(mb.x, mb.y, cam_tab + (int64_t)pair_cams[2 * p + 1] * TRI_CAM_STRIDE, r.z, r.w);
    und[o] = r;
}

// group k = pair * H + hypothesis: hyp_F (9 doubles, NaN when the pair has fewer than 8 rows) and hyp_ok
__global__ __launch_bounds__(256) void tv_hypothesis_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start,
                                                            const int32_t *__restrict__ pair_cams, const double *__restrict__ cam_tab,
                                                            const int64_t n_pairs, const int H, const uint64_t seed, double *__restrict__ hyp_F,
                                                            uint8_t *__restrict__ hyp_ok) {
    constexpr int G = 16;
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pairs * H) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t p = gid / H;
    const int h = (int)(gid - p * H);
    const int64_t s0 = start[p], n = start[p + 1] - s0;
    double F[9];
    bool ok = false;
    if (n >= TV_SAMPLE) {   // the same in every lane of the group
        int64_t pick[CONS_MAX_SAMPLE];
        cons_sample_positions(seed, (int32_t)p, n, h, TV_SAMPLE, pick);
        int64_t mine = 0;
#pragma unroll
        for (int i = 0; i < TV_SAMPLE; ++i)
            if (g == i) mine = pick[i];
        const TvCams k(cam_tab, pair_cams[2 * p], pair_cams[2 * p + 1]);
        const double4 m = und[s0 + mine];
        TvFit fit;
        ok = tv_eight_point<G>([&](auto &&f) { if (g < TV_SAMPLE) f(m); }, g, k, fit);
        tv_sandwich(k.inv_b(), fit.E, k.inv_a(), F);
#pragma unroll
        for (int i = 0; i < 9; ++i) ok = ok && isfinite(F[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = __builtin_nan("");
    }
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) hyp_F[9 * gid + i] = F[i];
        hyp_ok[gid] = ok ? 1 : 0;
    }
}

template <int G>
__global__ __launch_bounds__(256) void tv_score_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start, const int64_t n_pairs,
                                                       const int H, const double *__restrict__ hyp_F, const uint8_t *__restrict__ hyp_ok,
                                                       const double tau2, double *__restrict__ score) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pairs * H) return;
    const int64_t p = gid / H;
    const int64_t s0 = start[p], s1 = start[p + 1];
    double sum = INFINITY;
    if (hyp_ok[gid]) {   // the same in every lane of the group
        double F[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = hyp_F[9 * gid + i];
        sum = cons_truncated_sum<G>(s0, s1, g, tau2, [&](const int64_t o, bool &usable) {
            usable = true;   // a non-finite distance fails the comparison and counts as an outlier
            return tv_sampson(F, und[o]);
        });
    }
    if (g == 0) score[gid] = sum;
}

// sel (n_pairs, 2): inliers, winning hypothesis (-1: none); best: the winner's score (+inf: no usable hypothesis, NaN: too few rows)
template <int G>
__global__ __launch_bounds__(256) void tv_select_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start, const int64_t n_pairs,
                                                        const int32_t *__restrict__ order, const int H, const int n_min,
                                                        const double *__restrict__ hyp_F, const double *__restrict__ score, const double tau2,
                                                        uint8_t *__restrict__ flag, int32_t *__restrict__ sel, double *__restrict__ best_out) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pairs) return;
    const int64_t p = order[gid];
    const int64_t s0 = start[p], s1 = start[p + 1];
    double best = INFINITY;
    int best_k = INT32_MAX, n_fin;
    if (s1 - s0 >= n_min) cons_argmin<G>(score + p * H, H, g, best, best_k, n_fin, cons_count_none);
    if (best_k == INT32_MAX) {
        cons_flag_all<G>(s0, s1, g, flag, 0);
        if (g == 0) {
            sel[2 * p + 0] = 0; sel[2 * p + 1] = -1;
            best_out[p] = s1 - s0 >= n_min ? INFINITY : __builtin_nan("");
        }
        return;
    }
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = hyp_F[9 * (p * H + best_k) + i];
    const int cnt = cons_flag_inliers<G>(s0, s1, g, tau2, flag, [&](const int64_t o, bool &usable) {
        usable = true;
        return tv_sampson(F, und[o]);
    });
    if (g == 0) {
        sel[2 * p + 0] = cnt; sel[2 * p + 1] = best_k;
        best_out[p] = best;
    }
}

// T (n_pairs, 12) = [R | t] row-major, camera a -> camera b, |t| = 1; info (n_pairs, 5) = [n, inliers, front, status, winning hypothesis];
// stats (n_pairs, 3) = [score, RMS Sampson distance over the inliers, parallax].  A pair that is not OK has NaN in T, RMS and parallax.
template <int G>
__global__ __launch_bounds__(256) void tv_final_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start,
                                                       const int32_t *__restrict__ pair_cams, const double *__restrict__ cam_tab,
                                                       const int64_t n_pairs, const int32_t *__restrict__ order, const int n_min,
                                                       const uint8_t *__restrict__ flag, const int32_t *__restrict__ sel,
                                                       const double *__restrict__ best, double *__restrict__ T_out, int32_t *__restrict__ info,
                                                       double *__restrict__ stats) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pairs) return;
    const int64_t p = order[gid];
    const int64_t s0 = start[p], s1 = start[p + 1], n = s1 - s0;
    const int n_inl = sel[2 * p], hyp = sel[2 * p + 1];
    const double nan = __builtin_nan("");
    int status = TV_OK, n_front = 0;
    double T[12], rms = nan, parallax = nan;
    if (n < n_min) status = TV_TOO_FEW;
    else if (hyp < 0 || n_inl < TV_SAMPLE) status = TV_DEGENERATE;
    if (status == TV_OK) {   // the same in every lane of the group
        const TvCams k(cam_tab, pair_cams[2 * p], pair_cams[2 * p + 1]);
        TvFit fit;
        const bool ok = tv_eight_point<G>([&](auto &&f) {
            for (int64_t o = s0 + g; o < s1; o += G)
                if (flag[o]) f(und[o]);
        }, g, k, fit);
        if (!ok) status = TV_DEGENERATE;
        else {
            const TvAffine ia = k.inv_a(), ib = k.inv_b();
            double F[9];
            tv_sandwich(ib, fit.E, ia, F);
            // U = [u1 u2 u3], V = [v1 v2 v3], both proper: u_i = E v_i / sigma_i, u3 = u1 x u2, v3 = v1 x v2; W = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]:
            // R1 = U W V' = u2 v1' - u1 v2' + u3 v3', R2 = U W' V' = -u2 v1' + u1 v2' + u3 v3', t = +-u3
            double u1[3], u2[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                u1[i] = (fit.E0[3 * i] * fit.v1[0] + fit.E0[3 * i + 1] * fit.v1[1] + fit.E0[3 * i + 2] * fit.v1[2]) / fit.s1;
                u2[i] = (fit.E0[3 * i] * fit.v2[0] + fit.E0[3 * i + 1] * fit.v2[1] + fit.E0[3 * i + 2] * fit.v2[2]) / fit.s2;
            }
            double u3[3] = {u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]};
            const double v3[3] = {fit.v1[1] * fit.v2[2] - fit.v1[2] * fit.v2[1], fit.v1[2] * fit.v2[0] - fit.v1[0] * fit.v2[2],
                                  fit.v1[0] * fit.v2[1] - fit.v1[1] * fit.v2[0]};
            const double inv_t = 1.0 / sqrt(u3[0] * u3[0] + u3[1] * u3[1] + u3[2] * u3[2]);
#pragma unroll
            for (int i = 0; i < 3; ++i) u3[i] *= inv_t;
            double R1[9], R2[9];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const double d = u2[i] * fit.v1[j] - u1[i] * fit.v2[j], c = u3[i] * v3[j];
                    R1[3 * i + j] = c + d;
                    R2[3 * i + j] = c - d;
                }
            // one walk over the inliers: Sampson sum, and per candidate the count in front of both cameras and the squared ray angles.
            // Candidates 0: (R1, +t), 1: (R1, -t), 2: (R2, +t), 3: (R2, -t); the depths of -t are those of +t negated.
            int cnt[4] = {0, 0, 0, 0};
            double ang[4] = {0.0, 0.0, 0.0, 0.0}, e2sum = 0.0;
            for (int64_t o = s0 + g; o < s1; o += G) {
                if (!flag[o]) continue;
                const double4 m = und[o];
                e2sum += tv_sampson(F, m);
                const double xa = ia.p * m.x + ia.u, ya = ia.q * m.y + ia.v, xb = ib.p * m.z + ib.u, yb = ib.q * m.w + ib.v;
                const double bb = xb * xb + yb * yb + 1.0, bt = xb * u3[0] + yb * u3[1] + u3[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const double(&R)[9] = c == 0 ? R1 : R2;
                    const double r0 = R[0] * xa + R[1] * ya + R[2], r1 = R[3] * xa + R[4] * ya + R[5], r2 = R[6] * xa + R[7] * ya + R[8];
                    // normal equations of lambda_b x_b - lambda_a r = t: [[r.r, -r.b], [-r.b, b.b]] [la, lb]' = [-r.t, b.t]
                    const double rr = r0 * r0 + r1 * r1 + r2 * r2, rb = r0 * xb + r1 * yb + r2, rt = r0 * u3[0] + r1 * u3[1] + r2 * u3[2];
                    const double det = rr * bb - rb * rb, la = rb * bt - rt * bb, lb = rr * bt - rb * rt;
                    const double c0 = r1 - r2 * yb, c1 = r2 * xb - r0, c2 = r0 * yb - r1 * xb;   // r x b
                    const double a = atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), rb);
                    const bool pos = det > 0.0 && la > 0.0 && lb > 0.0, neg = det > 0.0 && la < 0.0 && lb < 0.0;
                    cnt[2 * c] += pos ? 1 : 0;
                    cnt[2 * c + 1] += neg ? 1 : 0;
                    ang[2 * c] += pos ? a * a : 0.0;
                    ang[2 * c + 1] += neg ? a * a : 0.0;
                }
            }
            e2sum = group_sum<G>(e2sum);
            int win = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                cnt[c] = group_sum<G>(cnt[c]);
                ang[c] = group_sum<G>(ang[c]);
            }
            double ang_w = ang[0];
            n_front = cnt[0];
#pragma unroll
            for (int c = 1; c < 4; ++c)
                if (cnt[c] > n_front) { n_front = cnt[c]; ang_w = ang[c]; win = c; }   // ties go to the lower candidate
            if (n_front == 0) status = TV_NO_CHEIRALITY;
            else {
                rms = sqrt(e2sum / (double)n_inl);
                parallax = sqrt(ang_w / (double)n_front);
                const double sgn = (win & 1) ? -1.0 : 1.0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) T[4 * i + j] = win < 2 ? R1[3 * i + j] : R2[3 * i + j];
                    T[4 * i + 3] = sgn * u3[i];
                }
                bool fin = isfinite(rms) && isfinite(parallax);
#pragma unroll
                for (int i = 0; i < 12; ++i) fin = fin && isfinite(T[i]);
                if (!fin) { status = TV_DEGENERATE; rms = nan; parallax = nan; }
            }
        }
    }
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) T_out[12 * p + i] = status == TV_OK ? T[i] : nan;
        info[5 * p + 0] = (int32_t)n; info[5 * p + 1] = n_inl; info[5 * p + 2] = n_front; info[5 * p + 3] = status; info[5 * p + 4] = hyp;
        stats[3 * p + 0] = best[p]; stats[3 * p + 1] = rms; stats[3 * p + 2] = parallax;
    }
}

}  // namespace pcs
