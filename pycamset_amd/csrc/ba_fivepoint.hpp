// ba_fivepoint.hpp — five-point hypotheses with a cheirality score, and the on-manifold refinement of a relative pose (SURVEY 8 row f10;
// pcs_twoview_set_solver).  The eight-point hypotheses of ba_twoview.hpp degenerate on coplanar points, the common scene of a calibration
// (boards, walls, floors); Nister's five-point solver does not.  Policy of DESIGN.md, "Batched handles", as in ba_twoview.hpp: group sums
// are xor-butterflies, no floating-point atomics, no scratch, every iteration count fixed, two runs agree bit for bit.
//
// tv5_hypothesis_kernel  one group of 16 lanes per (pair, hypothesis): five rows drawn by cons_sample_positions (sample size 5), rays in
//                        normalised camera coordinates, the four eigenvectors of the smallest eigenvalues of the 9 x 9 moment matrix
//                        (tv_sweep, the lane-distributed Jacobi of the eight-point fit), the ten cubic constraints as a 10 x 20 matrix
//                        with ONE ROW PER LANE, Gauss-Jordan with partial pivoting by shuffles, the degree-10 polynomial in z, its Sturm
//                        chain, and lane k bisects for the k-th smallest real root (TV5_BISECTIONS halvings of the
//                        Cauchy interval, TV5_POLISH Newton steps inside the bracket).  Lane k writes slot k: E, F and a usable flag.
// tv5_score_kernel<G>    one group per slot: the four (R, +-t) of E and, in ONE walk over the pair's rows, four sums min(e^2, tau^2) in
//                        which a row that is not in front of both cameras counts tau^2; the smallest (ties: lower candidate) is the
//                        slot's score, its (R, t) is written beside it.
// tv5_select_kernel<G>   one group per pair: the lowest score of all slots (ties: lower hypothesis, then lower root); inlier flags
//                        e^2 <= tau^2 and in front under the winner.
// tv5_final_kernel<G>    one group per pair: status, the winner's (R, t), RMS, parallax and the count in front over the inliers.
// tv_refine_kernel<G>    one group per pair, behind either final kernel: at most `iters` LM trials on R <- exp(omega) R, t <- exp(nu) t,
//                        nu in the tangent plane of t, over the signed Sampson residuals of the inliers with analytic Jacobians and the
//                        damping, accept and stop rules of triangulate_refine_kernel; RMS, parallax and the count in front again.
//
// Columns of the 10 x 20 (Nister): x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1.  After the elimination
// rows 4 .. 9 (e .. j) give k = e - z f, l = g - z h, m = i - z j, three rows [kx(z), ky(z), k1(z)] . (x, y, 1) = 0 of degrees (3, 3, 4);
// (p1, p2, p3) = k x l, the polynomial is p1 mx + p2 my + p3 m1 and x = p1 / p3, y = p2 / p3 at a root.
#pragma once
#include "ba_twoview.hpp"

namespace pcs {

constexpr int TV_SOLVER_EIGHT_POINT = 0, TV_SOLVER_FIVE_POINT = 1;
constexpr int TV5_SAMPLE = 5;
constexpr int TV5_SLOTS = 10;         // candidate slots per hypothesis: the real roots of the degree-10 polynomial, ascending
constexpr int TV5_MIN_INLIERS = 6;    // five rows fit any of the ten candidates: the sixth is the first that says something
constexpr int TV5_BISECTIONS = 56, TV5_POLISH = 4;
constexpr int TV_REFINE_MAX_ITERS = 50;
constexpr double TV_REFINE_LAMBDA0 = 1e-4, TV_REFINE_LAMBDA_MAX = 1e10, TV_REFINE_LAMBDA_MIN = 1e-15, TV_REFINE_FTOL = 1e-10, TV_REFINE_XTOL = 1e-10;

// ---- polynomials in (x, y, z): a linear one is [x, y, z, 1], a quadratic one is packed by pnp_tri over the same four "variables" ------
__host__ __device__ constexpr int tv5_column(const int a, const int b, const int c) {   // of the product of three variables (3: the one)
    const int code = 16 * ((a == 0) + (b == 0) + (c == 0)) + 4 * ((a == 1) + (b == 1) + (c == 1)) + ((a == 2) + (b == 2) + (c == 2));
    return code == 48 ? 0 : code == 12 ? 1 : code == 36 ? 2 : code == 24 ? 3 : code == 33 ? 4 : code == 32 ? 5 : code == 9 ? 6 : code == 8 ? 7
         : code == 21 ? 8 : code == 20 ? 9 : code == 18 ? 10 : code == 17 ? 11 : code == 16 ? 12 : code == 6 ? 13 : code == 5 ? 14 : code == 4 ? 15
         : code == 3 ? 16 : code == 2 ? 17 : code == 1 ? 18 : 19;
}

// q += s a b
__device__ __forceinline__ void tv5_mac11(const double (&a)[4], const double (&b)[4], const double s, double (&q)[10]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) q[i >= j ? pnp_tri(i, j) : pnp_tri(j, i)] += s * a[i] * b[j];
}

// row += s q l
__device__ __forceinline__ void tv5_mac21(const double (&q)[10], const double (&l)[4], const double s, double (&row)[20]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) row[tv5_column(i, j, c)] += s * q[pnp_tri(i, j)] * l[c];
}

template <int NA, int NB>
__device__ __forceinline__ void tv5_umac(const double (&a)[NA], const double (&b)[NB], const double s, double (&out)[NA + NB - 1]) {
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) out[i + j] += s * a[i] * b[j];
}

template <int N>
__device__ __forceinline__ double tv5_horner(const double (&c)[N], const double x) {
    double v = c[N - 1];
#pragma unroll
    for (int k = N - 2; k >= 0; --k) v = v * x + c[k];
    return v;
}

// The Sturm chain f0 = n, f1 = n', f(i+1) = -rem(f(i-1), f(i)), every remainder scaled to a largest |coefficient| of 1 (a positive factor
// changes no sign), kept as eleven polynomials of degrees 10 .. 0 in one array with compile-time offsets.  (The chain in quotient form,
// f(i+1) = q(i) f(i) - f(i-1) evaluated forwards, needs a third of the registers and is not stable: it miscounts near large roots.)
constexpr int TV5_CHAIN = 66;
__host__ __device__ constexpr int tv5_chain_at(const int i) { return 11 * i - i * (i - 1) / 2; }   // the first coefficient of f(i)

// one step of the construction: f(I - 1) of degree D + 1 and f(I) of degree D -> f(I + 1) = (a x + b) f(I) - f(I - 1), D = 10 - I
template <int I>
__device__ __forceinline__ void tv5_sturm_step(double (&c)[TV5_CHAIN]) {
    constexpr int D = 10 - I, o0 = tv5_chain_at(I - 1), o1 = tv5_chain_at(I), o2 = tv5_chain_at(I + 1);
    const double inv = 1.0 / c[o1 + D];
    const double a = c[o0 + D + 1] * inv;
    const double b = (c[o0 + D] - a * c[o1 + D - 1]) * inv;
    double big = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        c[o2 + k] = b * c[o1 + k] + (k > 0 ? a * c[o1 + (k > 0 ? k - 1 : 0)] : 0.0) - c[o0 + k];
        big = fmax(big, fabs(c[o2 + k]));
    }
    const double scale = 1.0 / big;
#pragma unroll
    for (int k = 0; k < D; ++k) c[o2 + k] *= scale;
    if constexpr (I < 9) tv5_sturm_step<I + 1>(c);
}

// sign changes of the chain at x (zeros and NaNs are skipped)
__device__ __forceinline__ int tv5_sign_changes(const double (&c)[TV5_CHAIN], const double x) {
    int last = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < 11; ++i) {
        double v = c[tv5_chain_at(i) + 10 - i];
#pragma unroll
        for (int k = 9 - i; k >= 0; --k) v = v * x + c[tv5_chain_at(i) + k];
        const int s = v > 0.0 ? 1 : (v < 0.0 ? -1 : 0);
        cnt += (s != 0 && last != 0 && s != last) ? 1 : 0;
        last = s != 0 ? s : last;
    }
    return cnt;
}

// rows e, f of the eliminated system (their last ten columns) -> [kx, ky, k1] of e - z f, ascending in z
__device__ __forceinline__ void tv5_row_pair(const double (&e)[10], const double (&f)[10], double (&kx)[4], double (&ky)[4], double (&k1)[5]) {
    kx[0] = e[2]; kx[1] = e[1] - f[2]; kx[2] = e[0] - f[1]; kx[3] = -f[0];
    ky[0] = e[5]; ky[1] = e[4] - f[5]; ky[2] = e[3] - f[4]; ky[3] = -f[3];
    k1[0] = e[9]; k1[1] = e[8] - f[9]; k1[2] = e[7] - f[8]; k1[3] = e[6] - f[7]; k1[4] = -f[6];
}

// group k = pair * H + hypothesis, slot = 10 k + root: hyp_E and hyp_F (9 doubles each, NaN when the pair has fewer than 5 rows), hyp_ok
__global__ __launch_bounds__(256) void tv5_hypothesis_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start,
                                                             const int32_t *__restrict__ pair_cams, const double *__restrict__ cam_tab,
                                                             const int64_t n_pairs, const int H, const uint64_t seed, double *__restrict__ hyp_E,
                                                             double *__restrict__ hyp_F, uint8_t *__restrict__ hyp_ok) {
    constexpr int G = 16;
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pairs * H) return;   // whole groups leave together; the shuffles below stay inside a group
    const int64_t p = gid / H;
    const int h = (int)(gid - p * H);
    const int64_t s0 = start[p], n = start[p + 1] - s0;
    const int64_t slot = gid * TV5_SLOTS + g;
    if (n < TV5_SAMPLE) {   // the same in every lane of the group
        if (g < TV5_SLOTS) {
#pragma unroll
            for (int i = 0; i < 9; ++i) hyp_E[9 * slot + i] = hyp_F[9 * slot + i] = __builtin_nan("");
            hyp_ok[slot] = 0;
        }
        return;
    }
    int64_t pick[CONS_MAX_SAMPLE];
    cons_sample_positions(seed, (int32_t)p, n, h, TV5_SAMPLE, pick);
    int64_t mine = 0;
#pragma unroll
    for (int i = 0; i < TV5_SAMPLE; ++i)
        if (g == i) mine = pick[i];
    const TvCams k(cam_tab, pair_cams[2 * p], pair_cams[2 * p + 1]);
    const TvAffine ia = k.inv_a(), ib = k.inv_b();
    // the 45 moments of the five constraint rows [xb xa, xb ya, xb, yb xa, yb ya, yb, xa, ya, 1] of x_b' E x_a = 0
    double A[9], V[9];
    {
        const double4 m = und[s0 + mine];
        const double w = g < TV5_SAMPLE ? 1.0 : 0.0;
        const double xa = ia.p * m.x + ia.u, ya = ia.q * m.y + ia.v, xb = ib.p * m.z + ib.u, yb = ib.q * m.w + ib.v;
        const double r[9] = {w * xb * xa, w * xb * ya, w * xb, w * yb * xa, w * yb * ya, w * yb, w * xa, w * ya, w};
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            A[c] = 0.0;
            V[c] = g == c ? 1.0 : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 9; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const double mij = group_sum<G>(r[i] * r[j]);
                if (g == i) A[j] = mij;
                if (g == j) A[i] = mij;
            }
    }
#pragma unroll 1
    for (int sweep = 0; sweep < TV_SWEEPS; ++sweep) tv_sweep<G>(A, V, g);
    double d[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) d[c] = __shfl(A[c], c, G);
    // the four columns of the smallest eigenvalues, in column order; the fifth smallest against the largest says whether the rows had rank 5
    bool ok = true;
    double dmax = d[0], fifth = 0.0;
    int col[4] = {0, 0, 0, 0}, n_sel = 0;
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        ok = ok && isfinite(d[c]);
        dmax = d[c] > dmax ? d[c] : dmax;
        int rank = 0;   // eigenvalues in front of this one (ties: the lower column first)
#pragma unroll
        for (int j = 0; j < 9; ++j) rank += (d[j] < d[c] || (d[j] == d[c] && j < c)) ? 1 : 0;
        if (rank == 4) fifth = d[c];
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (rank < 4 && n_sel == b) col[b] = c;
        n_sel += rank < 4 ? 1 : 0;
    }
    ok = ok && dmax > 0.0 && fifth > TV_RANK_RATIO * dmax;
    double Bs[4][9];   // the basis: E = x Bs[0] + y Bs[1] + z Bs[2] + Bs[3], every lane holds all of it
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const double mine_b = tv_pick(V, col[b]);   // V[g][col]: entry g of the eigenvector
#pragma unroll
        for (int e = 0; e < 9; ++e) Bs[b][e] = __shfl(mine_b, e, G);
    }
    // the constraint of this lane: lane 0 det E, lane 1 + 3 i + j the entry (i, j) of 2 E E' E - tr(E E') E; lanes 10 .. 15 hold zeros
    double row[20];
#pragma unroll
    for (int c = 0; c < 20; ++c) row[c] = 0.0;
    {
        double L[9][4];   // the nine entries of E as linear polynomials
#pragma unroll
        for (int e = 0; e < 9; ++e)
#pragma unroll
            for (int b = 0; b < 4; ++b) L[e][b] = Bs[b][e];
        if (g == 0) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {   // E[0][m] times the cofactor E[1][m1] E[2][m2] - E[1][m2] E[2][m1]
                const int m1 = (m + 1) % 3, m2 = (m + 2) % 3;
                double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                tv5_mac11(L[3 + m1], L[6 + m2], 1.0, q);
                tv5_mac11(L[3 + m2], L[6 + m1], -1.0, q);
                tv5_mac21(q, L[m], 1.0, row);
            }
        } else if (g < 10) {
            const int i = (g - 1) / 3, j = (g - 1) - 3 * i;
            double Ri[3][4], Cj[3][4], Eij[4];
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    Ri[m][b] = i == 0 ? L[m][b] : (i == 1 ? L[3 + m][b] : L[6 + m][b]);       // E[i][m]
                    Cj[m][b] = j == 0 ? L[3 * m][b] : (j == 1 ? L[3 * m + 1][b] : L[3 * m + 2][b]);   // E[m][j]
                }
#pragma unroll
            for (int b = 0; b < 4; ++b) Eij[b] = j == 0 ? Ri[0][b] : (j == 1 ? Ri[1][b] : Ri[2][b]);
            double tr[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int e = 0; e < 9; ++e) tv5_mac11(L[e], L[e], 1.0, tr);
            tv5_mac21(tr, Eij, -1.0, row);
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {   // 2 (E E')[i][kk] E[kk][j]
                double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int m = 0; m < 3; ++m) tv5_mac11(Ri[m], L[3 * kk + m], 1.0, q);
                tv5_mac21(q, Cj[kk], 2.0, row);
            }
        }
    }
    // Gauss-Jordan on the first ten columns: the pivot of column c is the largest |entry| of lanes c .. 9, ties to the lower lane
#pragma unroll
    for (int c = 0; c < 10; ++c) {
        double a = (g >= c && g < 10) ? (isfinite(row[c]) ? fabs(row[c]) : INFINITY) : -1.0;
        int piv = g;
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) {   // (|entry|, lane) is a total order: the maximum does not depend on the pairing
            const double oa = __shfl_xor(a, off, G);
            const int op = __shfl_xor(piv, off, G);
            if (oa > a || (oa == a && op < piv)) { a = oa; piv = op; }
        }
        ok = ok && a > 0.0 && a < INFINITY;
        const double inv = 1.0 / __shfl(row[c], piv, G);
        const double at_c = __shfl(row[c], c, G);   // every lane takes part in a shuffle: not inside the select below
        const double f = g == c ? 0.0 : (g == piv ? at_c : row[c]);   // this lane's entry of column c after the swap
#pragma unroll
        for (int kk = c; kk < 20; ++kk) {
            const double pr = __shfl(row[kk], piv, G) * inv, cr = __shfl(row[kk], c, G);
            const double mine_k = g == piv ? cr : row[kk];
            row[kk] = g == c ? pr : mine_k - f * pr;
        }
    }
    // rows e .. j to every lane, the hidden-variable polynomials
    double nz[11], p1[8], p2[8], p3[7];
    {
        double rw[6][10];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int kk = 0; kk < 10; ++kk) rw[r][kk] = __shfl(row[10 + kk], 4 + r, G);
        double kx[4], ky[4], k1[5], lx[4], ly[4], l1[5], mx[4], my[4], m1[5];
        tv5_row_pair(rw[0], rw[1], kx, ky, k1);
        tv5_row_pair(rw[2], rw[3], lx, ly, l1);
        tv5_row_pair(rw[4], rw[5], mx, my, m1);
#pragma unroll
        for (int i = 0; i < 8; ++i) p1[i] = p2[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 7; ++i) p3[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 11; ++i) nz[i] = 0.0;
        tv5_umac(ky, l1, 1.0, p1); tv5_umac(k1, ly, -1.0, p1);
        tv5_umac(k1, lx, 1.0, p2); tv5_umac(kx, l1, -1.0, p2);
        tv5_umac(kx, ly, 1.0, p3); tv5_umac(ky, lx, -1.0, p3);
        tv5_umac(p1, mx, 1.0, nz); tv5_umac(p2, my, 1.0, nz); tv5_umac(p3, m1, 1.0, nz);
    }
    // scale, Cauchy bound, derivative, the chain's quotients
    double nmax = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) nmax = fmax(nmax, fabs(nz[i]));
    const double nscale = 1.0 / nmax;
#pragma unroll
    for (int i = 0; i < 11; ++i) nz[i] *= nscale;
    const double ilead = 1.0 / nz[10];
    double bound = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) bound = fmax(bound, fabs(nz[i] * ilead));
    bound += 1.0;
    double dn[10], chain[TV5_CHAIN];
#pragma unroll
    for (int i = 0; i < 10; ++i) dn[i] = (double)(i + 1) * nz[i + 1];
#pragma unroll
    for (int i = 0; i < 11; ++i) chain[i] = nz[i];
#pragma unroll
    for (int i = 0; i < 10; ++i) chain[11 + i] = dn[i];
    tv5_sturm_step<1>(chain);
    ok = ok && isfinite(bound);
#pragma unroll
    for (int i = 0; i < TV5_CHAIN; ++i) ok = ok && isfinite(chain[i]);
    // lane k: the k-th smallest real root (the smallest z with at least k + 1 roots at or below it)
    double lo = -bound, hi = bound;
    const int at_lo = tv5_sign_changes(chain, lo);
    const int total = at_lo - tv5_sign_changes(chain, hi);
#pragma unroll 1
    for (int it = 0; it < TV5_BISECTIONS; ++it) {
        const double mid = (lo + hi) / 2.0;
        const bool above = at_lo - tv5_sign_changes(chain, mid) >= g + 1;
        lo = above ? lo : mid;
        hi = above ? mid : hi;
    }
    double z = (lo + hi) / 2.0;
#pragma unroll 1
    for (int it = 0; it < TV5_POLISH; ++it) {
        const double zn = z - tv5_horner(nz, z) / tv5_horner(dn, z);
        z = (isfinite(zn) && zn >= lo && zn <= hi) ? zn : z;
    }
    const double i3 = 1.0 / tv5_horner(p3, z);
    const double x = tv5_horner(p1, z) * i3, y = tv5_horner(p2, z) * i3;
    double E[9], F[9], e2 = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        E[i] = x * Bs[0][i] + y * Bs[1][i] + z * Bs[2][i] + Bs[3][i];
        e2 += E[i] * E[i];
    }
    const double ie = 1.0 / sqrt(e2);
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] *= ie;
    tv_sandwich(ib, E, ia, F);
    ok = ok && g < total && isfinite(z);
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && isfinite(E[i]) && isfinite(F[i]);
    if (g < TV5_SLOTS) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            hyp_E[9 * slot + i] = E[i];
            hyp_F[9 * slot + i] = F[i];
        }
        hyp_ok[slot] = ok ? 1 : 0;
    }
}

// ---- the four (R, +-t) of an essential matrix and the depth test, by the formulas of tv_final_kernel ---------------------------------
__device__ __forceinline__ void tv_decompose(const double (&E)[9], double (&R1)[9], double (&R2)[9], double (&u3)[3]) {
    double B[3][3], W3[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i][j] = E[i] * E[j] + E[3 + i] * E[3 + j] + E[6 + i] * E[6 + j];
    pnp_jacobi3(B, W3);
    const double e0 = B[0][0], e1 = B[1][1], e2 = B[2][2];
    const int k3 = e0 <= e1 && e0 <= e2 ? 0 : (e1 <= e2 ? 1 : 2);
    const double sg0 = sqrt(fmax(e0, 0.0)), sg1 = sqrt(fmax(e1, 0.0)), sg2 = sqrt(fmax(e2, 0.0));
    const double s1 = k3 == 0 ? sg1 : sg0, s2 = k3 == 2 ? sg1 : sg2;
    double v1[3], v2[3], u1[3], u2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v1[i] = k3 == 0 ? W3[i][1] : W3[i][0];
        v2[i] = k3 == 2 ? W3[i][1] : W3[i][2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        u1[i] = (E[3 * i] * v1[0] + E[3 * i + 1] * v1[1] + E[3 * i + 2] * v1[2]) / s1;
        u2[i] = (E[3 * i] * v2[0] + E[3 * i + 1] * v2[1] + E[3 * i + 2] * v2[2]) / s2;
    }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    const double v3[3] = {v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]};
    const double inv_t = 1.0 / sqrt(u3[0] * u3[0] + u3[1] * u3[1] + u3[2] * u3[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) u3[i] *= inv_t;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double dd = u2[i] * v1[j] - u1[i] * v2[j], c = u3[i] * v3[j];
            R1[3 * i + j] = c + dd;
            R2[3 * i + j] = c - dd;
        }
}

// pos / neg: in front of both cameras under (R, t) / (R, -t); ang (ANGLE only): the angle between the two rays
template <bool ANGLE>
__device__ __forceinline__ void tv_depth(const double (&R)[9], const double (&t)[3], const double xa, const double ya, const double xb, const double yb,
                                         bool &pos, bool &neg, double &ang) {
    const double bb = xb * xb + yb * yb + 1.0, bt = xb * t[0] + yb * t[1] + t[2];
    const double r0 = R[0] * xa + R[1] * ya + R[2], r1 = R[3] * xa + R[4] * ya + R[5], r2 = R[6] * xa + R[7] * ya + R[8];
    const double rr = r0 * r0 + r1 * r1 + r2 * r2, rb = r0 * xb + r1 * yb + r2, rt = r0 * t[0] + r1 * t[1] + r2 * t[2];
    const double det = rr * bb - rb * rb, la = rb * bt - rt * bb, lb = rr * bt - rb * rt;
    pos = det > 0.0 && la > 0.0 && lb > 0.0;
    neg = det > 0.0 && la < 0.0 && lb < 0.0;
    if constexpr (ANGLE) {
        const double c0 = r1 - r2 * yb, c1 = r2 * xb - r0, c2 = r0 * yb - r1 * xb;   // r x b
        ang = atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), rb);
    }
}

// slot k = (pair * H + hypothesis) * 10 + root: score (+inf: unusable) and slot_T (12 doubles) = [R | t] of the best of the four candidates
template <int G>
__global__ __launch_bounds__(256) void tv5_score_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start,
                                                        const int32_t *__restrict__ pair_cams, const double *__restrict__ cam_tab, const int64_t n_pairs,
                                                        const int HS, const double *__restrict__ hyp_E, const double *__restrict__ hyp_F,
                                                        const uint8_t *__restrict__ hyp_ok, const double tau2, double *__restrict__ score,
                                                        double *__restrict__ slot_T) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pairs * HS) return;
    const int64_t p = gid / HS;
    const int64_t s0 = start[p], s1 = start[p + 1];
    double best = INFINITY, T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = __builtin_nan("");
    if (hyp_ok[gid]) {   // the same in every lane of the group
        double E[9], F[9], R1[9], R2[9], u3[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            E[i] = hyp_E[9 * gid + i];
            F[i] = hyp_F[9 * gid + i];
        }
        tv_decompose(E, R1, R2, u3);
        const TvCams k(cam_tab, pair_cams[2 * p], pair_cams[2 * p + 1]);
        const TvAffine ia = k.inv_a(), ib = k.inv_b();
        // candidates 0: (R1, +t), 1: (R1, -t), 2: (R2, +t), 3: (R2, -t)
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t o = s0 + g; o < s1; o += G) {
            const double4 m = und[o];
            const double e2 = tv_sampson(F, m);
            const double capped = e2 <= tau2 ? e2 : tau2;   // a non-finite distance counts as an outlier
            const double xa = ia.p * m.x + ia.u, ya = ia.q * m.y + ia.v, xb = ib.p * m.z + ib.u, yb = ib.q * m.w + ib.v;
            bool pos, neg;
            double unused;
            tv_depth<false>(R1, u3, xa, ya, xb, yb, pos, neg, unused);
            sum[0] += pos ? capped : tau2;
            sum[1] += neg ? capped : tau2;
            tv_depth<false>(R2, u3, xa, ya, xb, yb, pos, neg, unused);
            sum[2] += pos ? capped : tau2;
            sum[3] += neg ? capped : tau2;
        }
        int win = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) sum[c] = group_sum<G>(sum[c]);
        best = sum[0];
#pragma unroll
        for (int c = 1; c < 4; ++c)
            if (sum[c] < best) { best = sum[c]; win = c; }   // ties go to the lower candidate
        const double sgn = (win & 1) ? -1.0 : 1.0;
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) T[4 * i + j] = win < 2 ? R1[3 * i + j] : R2[3 * i + j];
            T[4 * i + 3] = sgn * u3[i];
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) fin = fin && isfinite(T[i]);
        if (!fin || !(best < INFINITY)) best = INFINITY;
    }
    if (g == 0) {
        score[gid] = best;
#pragma unroll
        for (int i = 0; i < 12; ++i) slot_T[12 * gid + i] = T[i];
    }
}

// sel (n_pairs, 2): inliers, winning slot = 10 hypothesis + root (-1: none); best: the winner's score (+inf: no usable slot, NaN: too few rows)
template <int G>
__global__ __launch_bounds__(256) void tv5_select_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start,
                                                         const int32_t *__restrict__ pair_cams, const double *__restrict__ cam_tab, const int64_t n_pairs,
                                                         const int32_t *__restrict__ order, const int HS, const int n_min, const double *__restrict__ hyp_F,
                                                         const double *__restrict__ slot_T, const double *__restrict__ score, const double tau2,
                                                         uint8_t *__restrict__ flag, int32_t *__restrict__ sel, double *__restrict__ best_out) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pairs) return;
    const int64_t p = order[gid];
    const int64_t s0 = start[p], s1 = start[p + 1];
    double best = INFINITY;
    int best_k = INT32_MAX, n_fin;
    if (s1 - s0 >= n_min) cons_argmin<G>(score + p * HS, HS, g, best, best_k, n_fin, cons_count_none);
    if (best_k == INT32_MAX) {
        cons_flag_all<G>(s0, s1, g, flag, 0);
        if (g == 0) {
            sel[2 * p + 0] = 0; sel[2 * p + 1] = -1;
            best_out[p] = s1 - s0 >= n_min ? INFINITY : __builtin_nan("");
        }
        return;
    }
    const int64_t slot = p * HS + best_k;
    double F[9], R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = hyp_F[9 * slot + i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = slot_T[12 * slot + 4 * i + j];
        t[i] = slot_T[12 * slot + 4 * i + 3];
    }
    const TvCams k(cam_tab, pair_cams[2 * p], pair_cams[2 * p + 1]);
    const TvAffine ia = k.inv_a(), ib = k.inv_b();
    const int cnt = cons_flag_inliers<G>(s0, s1, g, tau2, flag, [&](const int64_t o, bool &usable) {   // usable: in front of both cameras
        const double4 m = und[o];
        const double xa = ia.p * m.x + ia.u, ya = ia.q * m.y + ia.v, xb = ib.p * m.z + ib.u, yb = ib.q * m.w + ib.v;
        bool neg;
        double unused;
        tv_depth<false>(R, t, xa, ya, xb, yb, usable, neg, unused);
        return tv_sampson(F, m);
    });
    if (g == 0) {
        sel[2 * p + 0] = cnt; sel[2 * p + 1] = best_k;
        best_out[p] = best;
    }
}

// F = K_b^-T [t]x R K_a^-1
__device__ __forceinline__ void tv_fundamental_of(const double (&R)[9], const double (&t)[3], const TvAffine &ia, const TvAffine &ib, double (&F)[9]) {
    double E[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        E[j] = -t[2] * R[3 + j] + t[1] * R[6 + j];
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        E[6 + j] = -t[1] * R[j] + t[0] * R[3 + j];
    }
    tv_sandwich(ib, E, ia, F);
}

// over the flagged rows of a pair at (R, t): the count in front of both cameras, the RMS Sampson distance, the RMS ray angle of the rows in front
template <int G>
__device__ __forceinline__ void tv_pose_stats(const double4 *__restrict__ und, const uint8_t *__restrict__ flag, const int64_t s0, const int64_t s1, const int g,
                                              const TvAffine &ia, const TvAffine &ib, const double (&R)[9], const double (&t)[3], int &n_front,
                                              double &rms, double &parallax) {
    double F[9];
    tv_fundamental_of(R, t, ia, ib, F);
    int cnt = 0, n_inl = 0;
    double ang = 0.0, e2sum = 0.0;
    for (int64_t o = s0 + g; o < s1; o += G) {
        if (!flag[o]) continue;
        const double4 m = und[o];
        const double xa = ia.p * m.x + ia.u, ya = ia.q * m.y + ia.v, xb = ib.p * m.z + ib.u, yb = ib.q * m.w + ib.v;
        bool pos, neg;
        double a;
        tv_depth<true>(R, t, xa, ya, xb, yb, pos, neg, a);
        e2sum += tv_sampson(F, m);
        n_inl += 1;
        cnt += pos ? 1 : 0;
        ang += pos ? a * a : 0.0;
    }
    n_front = group_sum<G>(cnt);
    n_inl = group_sum<G>(n_inl);
    rms = sqrt(group_sum<G>(e2sum) / (double)n_inl);
    parallax = sqrt(group_sum<G>(ang) / (double)n_front);
}

// the outputs of tv_final_kernel for the five-point path: the winner's (R, t) is the model (no refit over the inliers: it degenerates on a plane)
template <int G>
__global__ __launch_bounds__(256) void tv5_final_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start,
                                                        const int32_t *__restrict__ pair_cams, const double *__restrict__ cam_tab, const int64_t n_pairs,
                                                        const int32_t *__restrict__ order, const int HS, const int n_min, const uint8_t *__restrict__ flag,
                                                        const int32_t *__restrict__ sel, const double *__restrict__ best, const double *__restrict__ slot_T,
                                                        double *__restrict__ T_out, int32_t *__restrict__ info, double *__restrict__ stats) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (gid >= n_pairs) return;
    const int64_t p = order[gid];
    const int64_t s0 = start[p], s1 = start[p + 1], n = s1 - s0;
    const int n_inl = sel[2 * p], win = sel[2 * p + 1];
    const double nan = __builtin_nan("");
    int status = TV_OK, n_front = 0;
    double T[12], rms = nan, parallax = nan;
    if (n < n_min) status = TV_TOO_FEW;
    else if (win < 0 || n_inl < TV5_MIN_INLIERS) status = TV_DEGENERATE;
    if (status == TV_OK) {   // the same in every lane of the group
        const int64_t slot = p * HS + win;
        double R[9], t[3];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = slot_T[12 * slot + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) R[3 * i + j] = T[4 * i + j];
            t[i] = T[4 * i + 3];
        }
        const TvCams k(cam_tab, pair_cams[2 * p], pair_cams[2 * p + 1]);
        tv_pose_stats<G>(und, flag, s0, s1, g, k.inv_a(), k.inv_b(), R, t, n_front, rms, parallax);
        if (n_front == 0) { status = TV_NO_CHEIRALITY; rms = nan; parallax = nan; }
        else if (!(isfinite(rms) && isfinite(parallax))) { status = TV_DEGENERATE; rms = nan; parallax = nan; }
    }
    if (g == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) T_out[12 * p + i] = status == TV_OK ? T[i] : nan;
        info[5 * p + 0] = (int32_t)n; info[5 * p + 1] = n_inl; info[5 * p + 2] = n_front; info[5 * p + 3] = status;
        info[5 * p + 4] = win < 0 ? -1 : win / TV5_SLOTS;
        stats[3 * p + 0] = best[p]; stats[3 * p + 1] = rms; stats[3 * p + 2] = parallax;
    }
}

// ---- refinement ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void tv_mat3_mul(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

__device__ __forceinline__ void tv_cross_matrix(const double x, const double y, const double z, double (&K)[9]) {
    K[0] = 0.0; K[1] = -z; K[2] = y;
    K[3] = z; K[4] = 0.0; K[5] = -x;
    K[6] = -y; K[7] = x; K[8] = 0.0;
}

// exp of the rotation vector w: I + a K + b K K, a = sin(th) / th, b = 2 sin^2(th / 2) / th^2
__device__ __forceinline__ void tv_rodrigues(const double w0, const double w1, const double w2, double (&R)[9]) {
    const double th2 = w0 * w0 + w1 * w1 + w2 * w2, th = sqrt(th2);
    double a, b;
    if (th < 1e-8) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
    else {
        const double sh = sin(th / 2.0);
        a = sin(th) / th;
        b = 2.0 * sh * sh / th2;
    }
    double K[9], KK[9];
    tv_cross_matrix(w0, w1, w2, K);
    tv_mat3_mul(K, K, KK);
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = ((i & 3) == 0 ? 1.0 : 0.0) + a * K[i] + b * KK[i];
}

// two unit vectors that span the plane across t: b1 along e_k x t for the axis k of t's smallest |entry| (ties: lower k), b2 = t x b1
__device__ __forceinline__ void tv_tangent_basis(const double (&t)[3], double (&b1)[3], double (&b2)[3]) {
    const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
    const int k = a0 <= a1 && a0 <= a2 ? 0 : (a1 <= a2 ? 1 : 2);
    const double e0 = k == 0 ? 1.0 : 0.0, e1 = k == 1 ? 1.0 : 0.0, e2 = k == 2 ? 1.0 : 0.0;
    b1[0] = e1 * t[2] - e2 * t[1]; b1[1] = e2 * t[0] - e0 * t[2]; b1[2] = e0 * t[1] - e1 * t[0];
    const double inv = 1.0 / sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) b1[i] *= inv;
    b2[0] = t[1] * b1[2] - t[2] * b1[1]; b2[1] = t[2] * b1[0] - t[0] * b1[2]; b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// l0, l1 of G x_a, r0, r1 of G' x_b and x_b' G x_a: what the Sampson residual and its derivative along G need
__device__ __forceinline__ void tv_sampson_parts(const double (&Gm)[9], const double4 m, double &l0, double &l1, double &r0, double &r1, double &num) {
    l0 = Gm[0] * m.x + Gm[1] * m.y + Gm[2];
    l1 = Gm[3] * m.x + Gm[4] * m.y + Gm[5];
    const double l2 = Gm[6] * m.x + Gm[7] * m.y + Gm[8];
    r0 = Gm[0] * m.z + Gm[3] * m.w + Gm[6];
    r1 = Gm[1] * m.z + Gm[4] * m.w + Gm[7];
    num = m.z * l0 + m.w * l1 + l2;
}

constexpr int TV_REFINE_SUMS = 21;   // H (15, packed by pnp_tri) | J' r (5) | cost
// the sums of one pass over the flagged rows at (R, t): residual r = x_b' F x_a / sqrt(l0^2 + l1^2 + r0^2 + r1^2), parameters
// (omega, nu1, nu2) at zero with R <- exp(omega) R, t <- exp(nu1 b1 + nu2 b2) t
template <int G>
__device__ __forceinline__ void tv_refine_pass(const double4 *__restrict__ und, const uint8_t *__restrict__ flag, const int64_t s0, const int64_t s1, const int g,
                                               const TvAffine &ia, const TvAffine &ib, const double (&R)[9], const double (&t)[3], double (&s)[TV_REFINE_SUMS]) {
    double b1[3], b2[3], tx[9], F[9], dF[5][9];
    tv_tangent_basis(t, b1, b2);
    tv_cross_matrix(t[0], t[1], t[2], tx);
    {
        double E[9], K[9], KR[9];
        tv_mat3_mul(tx, R, E);
        tv_sandwich(ib, E, ia, F);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            tv_cross_matrix(k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, K);
            tv_mat3_mul(K, R, KR);
            tv_mat3_mul(tx, KR, E);
            tv_sandwich(ib, E, ia, dF[k]);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double(&b)[3] = k == 0 ? b1 : b2;
            tv_cross_matrix(b[1] * t[2] - b[2] * t[1], b[2] * t[0] - b[0] * t[2], b[0] * t[1] - b[1] * t[0], K);   // [b x t]x
            tv_mat3_mul(K, R, E);
            tv_sandwich(ib, E, ia, dF[3 + k]);
        }
    }
#pragma unroll
    for (int i = 0; i < TV_REFINE_SUMS; ++i) s[i] = 0.0;
    for (int64_t o = s0 + g; o < s1; o += G) {
        if (!flag[o]) continue;
        const double4 m = und[o];
        double l0, l1, r0, r1, num, J[5];
        tv_sampson_parts(F, m, l0, l1, r0, r1, num);
        const double ss = l0 * l0 + l1 * l1 + r0 * r0 + r1 * r1, inv = 1.0 / sqrt(ss), res = num * inv;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double d0, d1, e0, e1, dnum;
            tv_sampson_parts(dF[k], m, d0, d1, e0, e1, dnum);
            J[k] = dnum * inv - res * ((l0 * d0 + l1 * d1 + r0 * e0 + r1 * e1) / ss);
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
#pragma unroll
            for (int j = 0; j <= i; ++j) s[pnp_tri(i, j)] += J[i] * J[j];
            s[15 + i] += J[i] * res;
        }
        s[20] += res * res;
    }
#pragma unroll
    for (int i = 0; i < TV_REFINE_SUMS; ++i) s[i] = group_sum<G>(s[i]);
}

// Behind either final kernel: the pose of every OK pair is refined in place; n_front (info[2]), RMS and parallax (stats[1], stats[2]) are
// taken again at the refined pose.  A refined pose that is not finite or has no inlier in front leaves the unrefined outputs.
template <int G>
__global__ __launch_bounds__(256) void tv_refine_kernel(const double4 *__restrict__ und, const int64_t *__restrict__ start,
                                                        const int32_t *__restrict__ pair_cams, const double *__restrict__ cam_tab, const int64_t n_pairs,
                                                        const int32_t *__restrict__ order, const int iters, const uint8_t *__restrict__ flag,
                                                        double *__restrict__ T_out, int32_t *__restrict__ info, double *__restrict__ stats) {
    const int64_t gid = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    const bool live = gid < n_pairs;   // whole groups are live or dead; a dead group never takes part in a pass
    const int64_t p = order[live ? gid : n_pairs - 1];
    const int64_t s0 = start[p], s1 = start[p + 1];
    const TvCams k(cam_tab, pair_cams[2 * p], pair_cams[2 * p + 1]);
    const TvAffine ia = k.inv_a(), ib = k.inv_b();
    bool done = !live || info[5 * p + 3] != TV_OK;
    double R[9], t[3], H[15], gr[5], cost = 0.0, lam = TV_REFINE_LAMBDA0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = T_out[12 * p + 4 * i + j];
        t[i] = T_out[12 * p + 4 * i + 3];
    }
#pragma unroll
    for (int i = 0; i < 15; ++i) H[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) gr[i] = 0.0;
    const bool refined = !done;
    if (!done) {   // the same in every lane of the group
        double s[TV_REFINE_SUMS];
        tv_refine_pass<G>(und, flag, s0, s1, g, ia, ib, R, t, s);
#pragma unroll
        for (int i = 0; i < 15; ++i) H[i] = s[i];
#pragma unroll
        for (int i = 0; i < 5; ++i) gr[i] = -s[15 + i];
        cost = s[20];
        done = !isfinite(cost);
    }
    int it = 0;
    while (true) {
        double d[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        bool trial = false;
        if (!done) {
            double A[15];
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j) A[pnp_tri(i, j)] = i == j ? H[pnp_tri(i, i)] * (1.0 + lam) : H[pnp_tri(i, j)];
            if (it >= iters) done = true;
            else if (!pnp_ldl<5>(A, gr, d)) done = true;
            else trial = true;
        }
        if (!__any(trial)) break;   // a group's lanes agree; the wave leaves when no group has a trial left
        if (trial) {
            double b1[3], b2[3], dR[9], Rt[9], tt[3], s[TV_REFINE_SUMS];
            tv_tangent_basis(t, b1, b2);
            tv_rodrigues(d[0], d[1], d[2], dR);
            tv_mat3_mul(dR, R, Rt);
            tv_rodrigues(d[3] * b1[0] + d[4] * b2[0], d[3] * b1[1] + d[4] * b2[1], d[3] * b1[2] + d[4] * b2[2], dR);
#pragma unroll
            for (int i = 0; i < 3; ++i) tt[i] = dR[3 * i] * t[0] + dR[3 * i + 1] * t[1] + dR[3 * i + 2] * t[2];
            const double inv = 1.0 / sqrt(tt[0] * tt[0] + tt[1] * tt[1] + tt[2] * tt[2]);
#pragma unroll
            for (int i = 0; i < 3; ++i) tt[i] *= inv;
            tv_refine_pass<G>(und, flag, s0, s1, g, ia, ib, Rt, tt, s);
            ++it;
            const double step = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4]);
            const bool small = step <= TV_REFINE_XTOL * (TV_REFINE_XTOL + 1.0);
            if (s[20] < cost) {   // accepted (a NaN cost is not lower)
                const bool flat = cost - s[20] <= TV_REFINE_FTOL * cost;
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = Rt[i];
#pragma unroll
                for (int i = 0; i < 3; ++i) t[i] = tt[i];
#pragma unroll
                for (int i = 0; i < 15; ++i) H[i] = s[i];
#pragma unroll
                for (int i = 0; i < 5; ++i) gr[i] = -s[15 + i];
                cost = s[20];
                lam = fmax(lam * 0.1, TV_REFINE_LAMBDA_MIN);
                if (flat || small) done = true;
            } else {
                lam *= 10.0;
                if (small || lam > TV_REFINE_LAMBDA_MAX) done = true;
            }
        }
    }
    if (!refined) return;   // the same in every lane of the group
    int n_front;
    double rms, parallax;
    tv_pose_stats<G>(und, flag, s0, s1, g, ia, ib, R, t, n_front, rms, parallax);
    bool fin = n_front > 0 && isfinite(rms) && isfinite(parallax);
#pragma unroll
    for (int i = 0; i < 9; ++i) fin = fin && isfinite(R[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) fin = fin && isfinite(t[i]);
    if (g == 0 && fin) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) T_out[12 * p + 4 * i + j] = R[3 * i + j];
            T_out[12 * p + 4 * i + 3] = t[i];
        }
        info[5 * p + 2] = n_front;
        stats[3 * p + 1] = rms;
        stats[3 * p + 2] = parallax;
    }
}

}  // namespace pcs
