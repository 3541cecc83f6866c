// ba_group.hpp — reductions over a group of G lanes (G a power of two <= 64, groups aligned inside the wave): xor-butterflies, so every
// lane of the group ends with identical bits and nothing of a neighbouring group enters ("Batched handles").
#pragma once
#include <hip/hip_runtime.h>

namespace pcs {

template <int G>
__device__ __forceinline__ double group_sum(double x) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, G);
    return x;
}

template <int G>
__device__ __forceinline__ int group_sum(int x) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, G);
    return x;
}

// the minimum of (score, index) over the group, the lower index on equal scores.  (score, index) is a total order: the minimum does
// not depend on the pairing.
template <int G>
__device__ __forceinline__ void group_argmin(double &best, int &best_k) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const double os = __shfl_xor(best, off, G);
        const int ok = __shfl_xor(best_k, off, G);
        if (os < best || (os == best && ok < best_k)) { best = os; best_k = ok; }
    }
}

}  // namespace pcs
