// ba_prior.hpp — Gaussian parameter priors on a packed state [A | B | C | g | cost] (ba_schur.hpp, ba_normal.hpp).
//
// A prior is a list of entries (index i, mean mu_i, weight w_i = 1 / sigma_i > 0) over the parameter string p; the objective gains
// sum_i (w_i (p_i - mu_i))^2.  In the packed state that is w_i^2 on the diagonal entry of parameter i (A[i, i] for a leading column,
// the diagonal of its entity's C block for a trailing one), w_i^2 (p_i - mu_i) on g_i and the sum on the cost word.  The list holds
// every index once, so each diagonal and g destination has exactly ONE writer: plain adds.  The cost contribution is summed in an
// order that the list and the launch geometry fix — per thread over its entries, by lane exchange inside a wave, over the waves of a
// workgroup and over the workgroups in index order — in BOTH contraction modes: no floating-point atomics, the same bits on every run
// and on every rank of a sharded loop (which adds the prior behind its all-reduce, pcs_lm_trial_finish).
//
// A workgroup takes PRIOR_PER_WG = 1 024 entries (256 threads x 4).  Lists up to that length — the intrinsics of a rig, a few poses —
// are ONE launch of one workgroup that also adds its sum to the cost word.  Longer lists (the three million point coordinates of a
// free chain) take ceil(n / 1 024) workgroups that park their partial sums, and a second one-workgroup launch adds those to the cost
// word in workgroup order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_schur.hpp"

namespace pcs {

constexpr int PRIOR_THREADS = 256;
constexpr int PRIOR_PER_THREAD = 4;
constexpr int PRIOR_PER_WG = PRIOR_THREADS * PRIOR_PER_THREAD;

struct PriorArgs {
    const int64_t *idx;          // n entries: index into the parameter string, every index at most once
    const double *mean, *w;      // n each: mu_i and w_i = 1 / sigma_i > 0
    int64_t n;
    // the packed state and the parameter string it was built at.  With `sel` (an LM trial's finish half): two of each, the prior goes to
    // the TRIAL one, 1 - (*sel != 0), as lm_decide_kernel reads them; without: [0]
    double *packed[2];
    const double *ps[2];
    const int32_t *sel;
    const int32_t *stop;         // optional LM stop word (PCS_STOP_GUARD)
    int64_t n_lead, trail_off, c_off, g_off, n_params;   // layout: A is n_lead x n_lead; C starts c_off doubles in, g at g_off, the cost behind g
    int32_t tb;
    double *partial;             // gridDim.x > 1: one partial cost sum per workgroup; NULL: the one workgroup adds its sum to the cost word
    int32_t n_partial;           // prior_cost_kernel: how many
};

// the sum of 256 threads' values in a fixed order: lane exchange inside each wave, then the four waves in order (thread 0 holds the result)
__device__ __forceinline__ double prior_block_sum(double v, double *lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int wv = 0; wv < PRIOR_THREADS / 64; ++wv) s += lds[wv];
    }
    return s;
}

__global__ __launch_bounds__(PRIOR_THREADS) void prior_add_kernel(const PriorArgs a) {
    PCS_STOP_GUARD(a);
    __shared__ double lds[PRIOR_THREADS / 64];
    const int st = a.sel ? (*a.sel != 0 ? 0 : 1) : 0;
    double *pk = a.packed[st];
    const double *p = a.ps[st];
    double *g = pk + a.g_off;
    const int64_t base = (int64_t)blockIdx.x * PRIOR_PER_WG;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < PRIOR_PER_THREAD; ++j) {
        const int64_t k = base + (int64_t)j * PRIOR_THREADS + threadIdx.x;
        if (k >= a.n) break;
        const int64_t i = a.idx[k];
        if (i < 0 || i >= a.n_params) continue;   // (the host has checked the list; nothing is ever written outside the state)
        const double w = a.w[k], d = w * (p[i] - a.mean[k]);
        int64_t at;
        if (i < a.n_lead) {
            at = i * a.n_lead + i;
        } else {
            const int64_t t = i - a.trail_off, e = t / a.tb, c = t - e * a.tb;
            at = a.c_off + e * a.tb * a.tb + c * a.tb + c;
        }
        pk[at] += w * w;
        g[i] += w * d;
        acc += d * d;
    }
    const double s = prior_block_sum(acc, lds);
    if (threadIdx.x == 0) {
        if (a.partial) a.partial[blockIdx.x] = s;
        else g[a.n_params] += s;
    }
}

// cost word += the workgroups' partial sums, in workgroup order: thread t sums a contiguous run of them, then the threads in order
__global__ __launch_bounds__(PRIOR_THREADS) void prior_cost_kernel(const PriorArgs a) {
    PCS_STOP_GUARD(a);
    __shared__ double lds[PRIOR_THREADS];
    const int st = a.sel ? (*a.sel != 0 ? 0 : 1) : 0;
    const int per = (a.n_partial + PRIOR_THREADS - 1) / PRIOR_THREADS;
    const int k0 = (int)threadIdx.x * per, k1 = min(a.n_partial, k0 + per);
    double acc = 0.0;
    for (int k = k0; k < k1; ++k) acc += a.partial[k];
    lds[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < PRIOR_THREADS; ++t) s += lds[t];
        a.packed[st][a.g_off + a.n_params] += s;
    }
}

}  // namespace pcs
