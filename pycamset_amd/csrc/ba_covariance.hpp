// ba_covariance.hpp — the marginal covariance blocks of the parameters at a solution, from the pieces a Schur step leaves on the device.
//
// With H = J'J (linear loss, lambda = 0) split as in ba_schur.hpp, [A B; B' C], C_e = L_e L_e' per trailing entity, V = B L^-T and
// S = A - V V' = L L' (the lower triangle pcs_dense_spd_solve leaves in S):
//     Sigma_ll           = s2 S^-1,                 (S^-1)[b, b] = (L^-1[:, b])' (L^-1[:, b])
//     Sigma_ee           = s2 L_e^-T (I + Z_e' Z_e) L_e^-1,   Z = L^-1 V, Z_e = the tb columns of entity e
// Two kernels do it:
//   cov_trsm_kernel        X <- L^-1 X in place (X = V gives Z; the identity flag gives L^-1).  One workgroup per slab of 16 right-hand
//                          side columns, so the workgroups never wait for each other; per 16-row panel the four waves subtract the
//                          product of the panel's rows of L with the rows of X solved before it (v_mfma_f64_16x16x4, the K range split
//                          four ways and summed in a fixed order through LDS), then 16 lanes solve the 16 x 16 diagonal tile.  Only the
//                          lower triangle of L is read.  With the identity flag the zero rows of L^-1 above a slab are skipped.
//   cov_gram_kernel        out_b = X[r0_b:, c_b : c_b + w_b]' X[r0_b:, c_b : c_b + w_b], w_b <= 16: one workgroup per block, one
//                          v_mfma_f64_16x16x4 per four rows (the A and B operands are the same load), the four waves' partial sums
//                          added in a fixed order.  Optional epilogue: the sandwich L_e^-T (I + G) L_e^-1 with linvt (= L_e^-T), the
//                          scale s2, exact zeros at fixed parameters, and a symmetric result.
// No float atomics anywhere: two calls on the same input return the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcs {

constexpr int COV_NB = 16;
using cov_d4 = __attribute__((ext_vector_type(4))) double;

struct CovTrsmArgs {
    const double *L;     // n x n, row stride ldl: lower triangle (diagonal included); nothing above the diagonal is read
    double *X;           // n x m, row stride ldx: X <- L^-1 X in place
    int64_t ldl, ldx;
    int32_t n, m;
    int32_t identity;    // 1: X is not read; the result is L^-1 (m = n), zeros above the diagonal included
};

__global__ __launch_bounds__(256) void cov_trsm_kernel(const CovTrsmArgs a) {
    __shared__ double part[4][COV_NB][COV_NB + 1];
    __shared__ double Ld[COV_NB][COV_NB + 1];
    __shared__ double Xp[COV_NB][COV_NB + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ti = tid >> 4, tj = tid & 15;               // this thread's entry of a 16 x 16 tile
    const int c0 = blockIdx.x * COV_NB;                   // the slab's first column
    const int col = c0 + (lane & 15);                     // MFMA: column of the B operand and of the result
    const bool col_ok = col < a.m;
    const int p_begin = a.identity ? c0 : 0;              // column j of L^-1 is zero above row j
    if (a.identity && c0 + tj < a.m)
        for (int r = ti; r < p_begin; r += COV_NB) a.X[(int64_t)r * a.ldx + c0 + tj] = 0.0;
    for (int p0 = p_begin; p0 < a.n; p0 += COV_NB) {
        const int gr = p0 + ti, gc = c0 + tj;
        double xv = 0.0;
        if (gr < a.n && gc < a.m) xv = a.identity ? (gr == gc ? 1.0 : 0.0) : a.X[(int64_t)gr * a.ldx + gc];
        Ld[ti][tj] = (gr < a.n && tj <= ti) ? a.L[(int64_t)gr * a.ldl + p0 + tj] : (ti == tj ? 1.0 : 0.0);
        // the panel's update from the rows solved before it: sum over k in [p_begin, p0) of L[p0 + i][k] X[k][c0 + j]
        cov_d4 acc = {0.0, 0.0, 0.0, 0.0};
        const int arow = p0 + (lane & 15);
        const bool arow_ok = arow < a.n;
        const double *pa = a.L + (int64_t)(arow_ok ? arow : 0) * a.ldl + (lane >> 4);
        const double *pb = a.X + (int64_t)(lane >> 4) * a.ldx + (col_ok ? col : 0);
#pragma unroll 4
        for (int k = p_begin + 4 * wave; k < p0; k += 16) {   // p_begin and p0 are multiples of 16: k + 3 < p0 <= arow
            const double av = arow_ok ? pa[k] : 0.0;
            const double bv = col_ok ? pb[(int64_t)k * a.ldx] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave][(lane >> 4) + 4 * r][lane & 15] = acc[r];
        __syncthreads();
        Xp[ti][tj] = xv - (((part[0][ti][tj] + part[1][ti][tj]) + part[2][ti][tj]) + part[3][ti][tj]);
        __syncthreads();
        if (tid < COV_NB) {   // the diagonal tile: L_pp y = Xp, one column per lane
            double y[COV_NB];
#pragma unroll
            for (int i = 0; i < COV_NB; ++i) {
                double s = Xp[i][tid];
#pragma unroll
                for (int k = 0; k < i; ++k) s -= Ld[i][k] * y[k];
                y[i] = s / Ld[i][i];
            }
            if (c0 + tid < a.m) {
#pragma unroll
                for (int i = 0; i < COV_NB; ++i)
                    if (p0 + i < a.n) a.X[(int64_t)(p0 + i) * a.ldx + c0 + tid] = y[i];
            }
        }
        __threadfence_block();   // the panel's rows are operands of the next panels' updates in this workgroup
        __syncthreads();
    }
}

struct CovGramArgs {
    const double *X;                  // n_rows x n_cols, row stride ldx
    int64_t ldx;
    int32_t n_rows, n_cols, n_blocks;
    const int32_t *col, *width, *row0;   // per block: first column, width (1 .. 16), first row (row0 may be NULL: 0)
    double *out;                      // block b: out + b * out_stride, width x width row-major
    int64_t out_stride;
    // epilogue (all optional)
    const double *linvt;              // n_ent x tb x tb (L_e^-T, row-major): block b is entity col / tb -> L_e^-T (I + G) L_e^-1
    int32_t tb;
    const uint8_t *fixed;             // column c is parameter fixed_off + c: its row and column of the block are set to 0
    int64_t fixed_off;
    const double *scale_dev;          // the block is multiplied by scale * (*scale_dev, or 1 when NULL)
    double scale;
};

__global__ __launch_bounds__(256) void cov_gram_kernel(const CovGramArgs a) {
    __shared__ double part[4][COV_NB][COV_NB + 1];
    __shared__ double G[COV_NB][COV_NB + 1];
    __shared__ double T[COV_NB][COV_NB + 1];
    __shared__ double M[COV_NB][COV_NB + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ti = tid >> 4, tj = tid & 15;
    const int b = blockIdx.x;
    const int c = a.col[b], w = a.width[b], r0 = a.row0 ? a.row0[b] : 0;
    if (w < 1 || w > COV_NB) return;   // nothing can be written: the block's output size is not known
    double *out = a.out + (int64_t)b * a.out_stride;
    const bool sandwich = a.linvt != nullptr;
    const bool bad = c < 0 || c + w > a.n_cols || r0 < 0 || (sandwich && (w != a.tb || c % a.tb != 0));
    if (bad) {   // a malformed descriptor: the block says so instead of reading outside X
        if (ti < w && tj < w) out[ti * w + tj] = __builtin_nan("");
        return;
    }
    const int i = lane & 15;
    const bool ok = i < w;
    cov_d4 acc = {0.0, 0.0, 0.0, 0.0};
    const double *px = a.X + (ok ? c + i : c);
#pragma unroll 4
    for (int k = r0 + 4 * wave; k < a.n_rows; k += 16) {
        const int row = k + (lane >> 4);
        const double v = (ok && row < a.n_rows) ? px[(int64_t)row * a.ldx] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v, v, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][(lane >> 4) + 4 * r][lane & 15] = acc[r];
    __syncthreads();
    G[ti][tj] = ((part[0][ti][tj] + part[1][ti][tj]) + part[2][ti][tj]) + part[3][ti][tj];
    if (sandwich) {
        const int64_t e = c / a.tb;
        T[ti][tj] = (ti < w && tj < w) ? a.linvt[(e * a.tb + ti) * a.tb + tj] : 0.0;
    }
    __syncthreads();
    double v = G[ti][tj];
    if (sandwich) {   // T (I + G) T' in two products through LDS
        double s = 0.0;
        for (int k = 0; k < w; ++k) s += T[ti][k] * (G[k][tj] + (k == tj ? 1.0 : 0.0));
        M[ti][tj] = s;
        __syncthreads();
        s = 0.0;
        for (int k = 0; k < w; ++k) s += M[ti][k] * T[tj][k];
        v = s;
    }
    const double s2 = a.scale * (a.scale_dev ? *a.scale_dev : 1.0);
    __syncthreads();
    G[ti][tj] = v * s2;
    __syncthreads();
    if (ti < w && tj < w) {
        double r = 0.5 * (G[ti][tj] + G[tj][ti]);   // exactly symmetric
        if (a.fixed && (a.fixed[a.fixed_off + c + ti] || a.fixed[a.fixed_off + c + tj])) r = 0.0;
        out[ti * w + tj] = r;
    }
}

}  // namespace pcs
