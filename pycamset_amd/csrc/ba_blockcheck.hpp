// ba_blockcheck.hpp — the device Jacobian check of ONE user block (abstract_function_block.test_self; the counterpart of the reference's
// test_self, abstract_function_blocks.py:750-775, on the GPU and on the block's own device bodies).
//
// pycamset_amd/chain_compiler.py (blockcheck_source) emits a translation unit with the block's `struct user::<name>` — device strings
// or bodies translated from Python, exactly as a chain pastes them — and PCS_BLOCKCHECK_ENTRY_POINTS(user::<name>, TEMPLATED); it is
// compiled and cached like a chain and driven by pcs_blockcheck (include/pcs_hip.h).
//
// One thread per (point, column) pair.  A point row is [params(NP), inp(NINROW)]: NINROW = NIN, or 3 for a templated source (its
// `inp` is the template point, not differentiated).  Column -1 writes fun and jac at the point; column j >= 0 writes the
// fourth-order central difference of fun in row entry j,
//     fd_j = (f(x - 2h) - 8 f(x - h) + 8 f(x + h) - f(x + 2h)) / (12 h),   h = eps^(1/5) max(1, |x_j|)  (rounded to a representable step).
// Every private array is indexed by compile-time constants only (the perturbed entry is selected, not addressed): no scratch.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>

#include <cstdint>
#else
#include "ba_rtc_prelude.hpp"
#endif

#include "ba_device.hpp"   // what a user body may call in a chain, it may call here: pcs::rot_terms / pcs::rot_element (Rodrigues rotation and its derivative)

namespace pcs {

struct BlockcheckArgs {
    const double *pts;   // m x (NP + NINROW)
    int64_t m;
    double *fun;         // m x NOUT
    double *jac;         // m x NOUT x (NP + NIN)
    double *fd;          // m x NOUT x (NP + NIN)
};

template <class U, bool TEMPLATED>
__device__ __forceinline__ void blockcheck_body(const BlockcheckArgs &a) {
    constexpr int NP = U::NP, NIN = U::NIN, NOUT = U::NOUT;
    constexpr int NINROW = TEMPLATED ? 3 : NIN, NR = NP + NINROW, NC = NP + NIN;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.m * (NC + 1)) return;
    const int64_t pt = t / (NC + 1);
    const int col = (int)(t - pt * (NC + 1)) - 1;
    const double *row = a.pts + pt * NR;
    double p[NP], x[NINROW > 0 ? NINROW : 1];
#pragma unroll
    for (int j = 0; j < NP; ++j) p[j] = row[j];
#pragma unroll
    for (int j = 0; j < NINROW; ++j) x[j] = row[NP + j];
    if (col < 0) {
        double f[NOUT], J[NOUT * NC];
        U::fun(p, x, f);
        U::jac(p, x, J);
#pragma unroll
        for (int o = 0; o < NOUT; ++o) a.fun[pt * NOUT + o] = f[o];
#pragma unroll
        for (int q = 0; q < NOUT * NC; ++q) a.jac[pt * NOUT * NC + q] = J[q];
        return;
    }
    const double xj = row[col];
    const double h0 = 7.400828044922853e-4 * fmax(1.0, fabs(xj));   // eps^(1/5), eps = 2^-52
    const double h = (xj + h0) - xj;
    const double step[4] = {-2.0 * h, -h, h, 2.0 * h};
    const double wt[4] = {1.0, -8.0, 8.0, -1.0};
    double acc[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) acc[o] = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        double ps[NP], xs[NINROW > 0 ? NINROW : 1], f[NOUT];
#pragma unroll
        for (int j = 0; j < NP; ++j) ps[j] = j == col ? xj + step[s] : p[j];
#pragma unroll
        for (int j = 0; j < NINROW; ++j) xs[j] = (!TEMPLATED && NP + j == col) ? xj + step[s] : x[j];
        U::fun(ps, xs, f);
#pragma unroll
        for (int o = 0; o < NOUT; ++o) acc[o] += wt[s] * f[o];
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) a.fd[(pt * NOUT + o) * NC + col] = acc[o] / (12.0 * h);
}

}  // namespace pcs

// the shape the code object was built for: {NP, NIN, NOUT, TEMPLATED}, read back by pcs_blockcheck before it launches
#define PCS_BLOCKCHECK_ENTRY_POINTS(U, TEMPLATED)                                                                 \
    extern "C" __device__ const int pcs_blockcheck_shape[4] = {U::NP, U::NIN, U::NOUT, (TEMPLATED) ? 1 : 0};     \
    extern "C" __global__ __launch_bounds__(256) void pcs_blockcheck(const pcs::BlockcheckArgs a) { pcs::blockcheck_body<U, (TEMPLATED)>(a); }
