// ba_bounds.hpp — box bounds lo <= x <= hi on the parameter string in the device LM trial (SURVEY 8 row f2+b).
//
// An active set plus a step truncated at the first bound: the two pieces that keep the identity (H + lambda D) d = -g on the free
// parameters, which lm_decide_kernel's predicted reduction rests on, and that need no product with the packed H.
//
//   bounds_active_kernel    from the CURRENT state (string x, gradient g of the packed state the selector names):
//                               fixed_eff[i] = fixed[i] || lo_i == hi_i || (x_i <= lo_i && g_i > 0) || (x_i >= hi_i && g_i < 0)
//                                              || (pin[i] && x_i on a bound)
//                           and the number of entries the bounds added to the caller's mask.  The Schur step then reads fixed_eff
//                           where it read fixed: identity rows and columns, zero gradient, zero step.  A parameter leaves the set
//                           when its gradient turns inward; the only memory is `pin` (below).
//   bounds_truncate_kernel  behind the step d and the trial string, in front of the build:
//                               alpha = min(1, min_i alpha_i),  alpha_i = (bound_i - x_i) / d_i for the bound d_i moves towards
//                               x_new = min(max(x + alpha d, lo), hi),  delta = x_new - x
//                           The entry that sets alpha lands on its bound exactly (ties: the lowest index).  With alpha = 1 an entry
//                           no bound touches keeps the bits of delta and of the trial string the step wrote.
//                           An entry that sits ON a bound and whose step points out of the box (its gradient points in, so it is not
//                           in the active set, but the coupled step disagrees) would make alpha = 0 and stall the loop: it is PINNED
//                           instead — its own component of the step is dropped, it takes no part in alpha, and pin[i] is set: a step
//                           with a component dropped is a poor one, so if the trial is rejected the NEXT trial holds the entry in
//                           its active set and solves the properly reduced system.  lm_decide_kernel clears the pins when it
//                           accepts a trial: the entry is then free to be tested again from the new state.
// Both are ONE workgroup of 1 024 threads striding over n_params (at most 65 535: 64 strides): a trial spends two short launches on
// its bounds.  The minimum and its index go through a fixed tree in LDS, the count through a fixed order of lanes and waves: the same
// bits and the same index on every run and on every rank of a sharded loop.  Plain vector loads and stores, no atomics; both start
// with the stop word like every kernel of a trial, and both follow the state selector the way the Schur step does.
// alpha_i and x + alpha d are computed with separate roundings (no contraction), so a NumPy restatement gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_schur.hpp"

namespace pcs {

constexpr int BOUNDS_THREADS = 1024;
constexpr int BOUNDS_LOG_TRIALS = 4096;      // per-trial records (alpha, active count) the decision keeps for the host (BoundStore)

struct BoundsArgs {
    const double *lo, *hi;       // n_params each; -inf / +inf = none
    const uint8_t *fixed;        // the caller's mask
    uint8_t *fixed_eff;          // bounds_active_kernel: out
    uint8_t *pin;                // n_params bytes of the handle: set by bounds_truncate_kernel, read by bounds_active_kernel, cleared by an accepted trial
    // the two parameter strings and (bounds_active_kernel) the gradients of the two packed states; the CURRENT one is *sel != 0 ? 1 : 0
    // (0 without sel), the trial string is the other one
    double *ps[2];
    const double *g[2];
    double *delta;               // bounds_truncate_kernel: in / out
    double *alpha;               // bounds_truncate_kernel: out, one word
    int32_t *n_active;           // bounds_active_kernel: out, one word
    const int32_t *sel, *stop;
    int64_t n_params;
};

__global__ __launch_bounds__(BOUNDS_THREADS) void bounds_active_kernel(const BoundsArgs a) {
    PCS_STOP_GUARD(a);
    __shared__ int32_t cnt[BOUNDS_THREADS / 64];
    const int tid = threadIdx.x;
    const int cur = a.sel ? (*a.sel != 0 ? 1 : 0) : 0;
    const double *x = a.ps[cur], *g = a.g[cur];
    int32_t n = 0;
    for (int64_t i = tid; i < a.n_params; i += BOUNDS_THREADS) {
        const double xi = x[i], gi = g[i], lo = a.lo[i], hi = a.hi[i];
        const bool user = a.fixed[i] != 0;
        const bool held = a.pin[i] != 0 && (xi <= lo || xi >= hi);
        const bool bound = lo == hi || (xi <= lo && gi > 0.0) || (xi >= hi && gi < 0.0) || held;
        a.fixed_eff[i] = (user || bound) ? 1 : 0;
        n += (!user && bound) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((tid & 63) == 0) cnt[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        int32_t s = 0;
#pragma unroll
        for (int w = 0; w < BOUNDS_THREADS / 64; ++w) s += cnt[w];
        *a.n_active = s;
    }
}

// on (or beyond) a bound with the step pointing out of the box: the component is dropped
__device__ __forceinline__ bool bounds_pinned(const double x, const double d, const double lo, const double hi) {
    return (d > 0.0 && x >= hi) || (d < 0.0 && x <= lo);
}
// the fraction of d that takes x to the bound d moves towards (+inf: none in that direction, or pinned)
__device__ __forceinline__ double bounds_fraction(const double x, const double d, const double lo, const double hi) {
#pragma clang fp contract(off)
    double f = __builtin_inf();
    if (bounds_pinned(x, d, lo, hi)) return f;
    if (d > 0.0 && hi < __builtin_inf()) f = (hi - x) / d;
    else if (d < 0.0 && lo > -__builtin_inf()) f = (lo - x) / d;
    return f;
}
__device__ __forceinline__ double bounds_moved(const double x, const double alpha, const double d) {
#pragma clang fp contract(off)
    const double p = alpha * d;
    return x + p;
}

__global__ __launch_bounds__(BOUNDS_THREADS) void bounds_truncate_kernel(const BoundsArgs a) {
    PCS_STOP_GUARD(a);
    __shared__ double sv[BOUNDS_THREADS];
    __shared__ int32_t si[BOUNDS_THREADS];
    const int tid = threadIdx.x;
    const int cur = a.sel ? (*a.sel != 0 ? 1 : 0) : 0;
    const double *x = a.ps[cur];
    double *xn = a.ps[1 - cur];
    double best = __builtin_inf();
    int32_t at = INT32_MAX;
    for (int64_t i = tid; i < a.n_params; i += BOUNDS_THREADS) {   // rising i: the first of equal fractions stays
        const double f = bounds_fraction(x[i], a.delta[i], a.lo[i], a.hi[i]);
        if (f < best) { best = f; at = (int32_t)i; }
    }
    sv[tid] = best;
    si[tid] = at;
    __syncthreads();
    for (int half = BOUNDS_THREADS / 2; half > 0; half >>= 1) {      // the fixed tree: the smaller fraction, of equal ones the lower index
        if (tid < half) {
            const double v = sv[tid + half];
            const int32_t j = si[tid + half];
            if (v < sv[tid] || (v == sv[tid] && j < si[tid])) { sv[tid] = v; si[tid] = j; }
        }
        __syncthreads();
    }
    const bool cut = sv[0] < 1.0;
    const double alpha = cut ? sv[0] : 1.0;
    const int32_t hit = cut ? si[0] : -1;
    if (tid == 0) *a.alpha = alpha;
    for (int64_t i = tid; i < a.n_params; i += BOUNDS_THREADS) {
        const double xi = x[i], d = a.delta[i], lo = a.lo[i], hi = a.hi[i];
        const bool pinned = bounds_pinned(xi, d, lo, hi);
        if (pinned) a.pin[i] = 1;
        const double t = bounds_moved(xi, alpha, pinned ? 0.0 : d);
        double c = fmin(fmax(t, lo), hi);
        if ((int32_t)i == hit) c = d > 0.0 ? hi : lo;
        if (t != t || (!cut && !pinned && c == t)) continue;   // the whole step and no bound in the way (or a void step): delta and the trial entry keep the step's bits
        a.delta[i] = c - xi;
        xn[i] = c;
    }
}

}  // namespace pcs
