// ba_consensus.hpp — what the consensus stages share: target pose (ba_pnp_consensus.hpp), triangulation (ba_tri_consensus.hpp), planar
// homography (ba_intr_consensus.hpp), two-view eight-point (ba_twoview.hpp) and five-point (ba_fivepoint.hpp), 3-D registration
// (ba_align.hpp).  Every stage draws a fixed number of samples, fits a candidate to each, scores every candidate on all rows of its
// problem by a truncated squared error, takes the lowest score and flags the rows within the threshold of the winner; three of them
// then compact the table to the flagged rows.  A stage keeps its own kernels (signature, guards, output record, the error of a row);
// the walks below are the part that is the same, as lane-level templates that take the stage's error as a callable.  Policy of
// DESIGN.md, "Batched handles": lane g of a group of G owns rows g, g + G, ...; group sums are xor-butterflies (ba_group.hpp); every
// sum in a fixed order; the sample count is fixed: two runs agree bit for bit.
//
// cons_mix64, cons_sample_positions   the counter-based generator (a splitmix64 finaliser: 64-bit multiplies, shifts, xors) and the
//                            sample of a hypothesis: a partial Fisher-Yates keyed by (seed, stream, rows of the problem, hypothesis).
// cons_truncated_sum         the score of one candidate: sum of min(e^2, tau^2), tau^2 for a row that is not usable.
// cons_argmin                the winner of a problem: the lowest score, ties to the lower candidate; how many candidates count as finite.
// cons_flag_all, cons_flag_inliers   one flag per row: a constant, or usable and e^2 <= tau^2; the inlier count.
// cons_count_scan_kernel     exclusive scan of the counts in cinfo[4 j] (integers: any order gives the same sums): one workgroup of 1 024
//                            threads, each with a contiguous stretch of the problems: its sum, a scan of the 1 024 sums, its stretch again.
// cons_compact_kernel        stable scatter of the flagged rows by ballot and popcount: the order inside a problem is preserved.
// cons_restore_count_kernel  the full row count of every problem back into a column of an info table (the estimator behind the stage
//                            saw the compacted table and wrote the inlier count there).
#pragma once
#include <hip/hip_runtime.h>

#include "ba_group.hpp"

namespace pcs {

constexpr int CONS_MAX_SAMPLE = 16;   // positions of a sample stay in registers (every index a compile-time constant)

__device__ __forceinline__ uint64_t cons_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
constexpr uint64_t CONS_GOLDEN = 0x9e3779b97f4a7c15ull;

// the sample of hypothesis h in a problem of n rows of stream cam: S distinct positions in [0, n), ascending in pick[0 .. S)
__device__ __forceinline__ void cons_sample_positions(const uint64_t seed, const int32_t cam, const int64_t n, const int h, const int S,
                                                      int64_t (&pick)[CONS_MAX_SAMPLE]) {
    uint64_t k = cons_mix64(seed + CONS_GOLDEN);
    k = cons_mix64(k ^ (uint64_t)(uint32_t)cam);
    k = cons_mix64(k ^ (uint64_t)n);
    k = cons_mix64(k ^ (uint64_t)(uint32_t)h);
    // partial Fisher-Yates on the identity permutation, kept sparse: step i swaps positions i and j >= i; mj[i] = j now holds mv[i]
    int64_t mj[CONS_MAX_SAMPLE], mv[CONS_MAX_SAMPLE];
#pragma unroll
    for (int i = 0; i < CONS_MAX_SAMPLE; ++i) {
        pick[i] = INT64_MAX;
        mj[i] = -1;
        mv[i] = 0;
        if (i < S) {
            const uint64_t r = cons_mix64(k + (uint64_t)(i + 1) * CONS_GOLDEN);
            const int64_t j = i + (int64_t)(r % (uint64_t)(n - i));
            int64_t vi = i, vj = j;
#pragma unroll
            for (int m = 0; m < i; ++m) {   // the latest entry of a position wins
                if (mj[m] == i) vi = mv[m];
                if (mj[m] == j) vj = mv[m];
            }
            mj[i] = j;
            mv[i] = vi;
            pick[i] = vj;
        }
    }
    // ascending: odd-even transposition (the unused tail holds INT64_MAX and stays behind)
#pragma unroll
    for (int round = 0; round < CONS_MAX_SAMPLE; ++round)
#pragma unroll
        for (int i = round & 1; i + 1 < CONS_MAX_SAMPLE; i += 2) {
            const int64_t a = pick[i], b = pick[i + 1];
            pick[i] = a < b ? a : b;
            pick[i + 1] = a < b ? b : a;
        }
}

// The walks.  [s0, s1) are the rows of the problem, g the lane inside its group; e2_of(o, usable) returns the squared error of row o at
// the candidate and sets `usable` (false: the row counts as an outlier whatever e2 is).  Every lane of the group must call them.

// sum of usable && e2 <= tau2 ? e2 : tau2 over the rows, the same bits in every lane
template <int G, class E2>
__device__ __forceinline__ double cons_truncated_sum(const int64_t s0, const int64_t s1, const int g, const double tau2, E2 &&e2_of) {
    double sum = 0.0;
    for (int64_t o = s0 + g; o < s1; o += G) {
        bool usable;
        const double e2 = e2_of(o, usable);
        sum += usable && e2 <= tau2 ? e2 : tau2;
    }
    return group_sum<G>(sum);
}

// the lowest of score[0 .. n) and its index (INT32_MAX: none below +inf); n_fin: the candidates k with counted(k, score[k])
template <int G, class Counted>
__device__ __forceinline__ void cons_argmin(const double *__restrict__ score, const int n, const int g, double &best, int &best_k, int &n_fin,
                                            Counted &&counted) {
    best = INFINITY;
    best_k = INT32_MAX;
    n_fin = 0;
    for (int k = g; k < n; k += G) {   // ascending inside a lane: of equal scores the lower candidate stays
        const double s = score[k];
        if (s < best) { best = s; best_k = k; }
        n_fin += counted(k, s) ? 1 : 0;
    }
    group_argmin<G>(best, best_k);
    n_fin = group_sum<G>(n_fin);
}
// for a stage that reports no count of finite candidates
__device__ __forceinline__ bool cons_count_none(int, double) { return false; }

template <int G>
__device__ __forceinline__ void cons_flag_all(const int64_t s0, const int64_t s1, const int g, uint8_t *__restrict__ flag, const uint8_t value) {
    for (int64_t o = s0 + g; o < s1; o += G) flag[o] = value;
}

// flag[o] = usable && e2 <= tau2 (flag = NULL: nothing is written); returns the number of such rows, the same in every lane
template <int G, class E2>
__device__ __forceinline__ int cons_flag_inliers(const int64_t s0, const int64_t s1, const int g, const double tau2, uint8_t *__restrict__ flag,
                                                 E2 &&e2_of) {
    int cnt = 0;
    for (int64_t o = s0 + g; o < s1; o += G) {
        bool usable;
        const double e2 = e2_of(o, usable);
        const bool in = usable && e2 <= tau2;
        if (flag) flag[o] = in ? 1 : 0;
        cnt += in ? 1 : 0;
    }
    return group_sum<G>(cnt);
}

// c_start[j] = sum of cinfo[4 i] over i < j, c_start[n] = the total.  Launched as ONE workgroup of CONS_SCAN_THREADS.
constexpr int CONS_SCAN_THREADS = 1024;
__global__ __launch_bounds__(CONS_SCAN_THREADS) void cons_count_scan_kernel(const int32_t *__restrict__ cinfo, const int64_t n, int64_t *__restrict__ c_start) {
    __shared__ int64_t sm[CONS_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t chunk = (n + CONS_SCAN_THREADS - 1) / CONS_SCAN_THREADS;
    const int64_t lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += (int64_t)cinfo[4 * i];
    sm[t] = sum;
    __syncthreads();
    for (int off = 1; off < CONS_SCAN_THREADS; off <<= 1) {
        const int64_t add = t >= off ? sm[t - off] : 0;
        __syncthreads();
        sm[t] += add;
        __syncthreads();
    }
    int64_t run = sm[t] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        c_start[i] = run;
        run += (int64_t)cinfo[4 * i];
    }
    if (t == CONS_SCAN_THREADS - 1) c_start[n] = sm[t];
}

// one group per problem: the flagged rows to [c_start[j], c_start[j + 1]) in their order.  The ballot is the wave's; a group reads its own G bits.
template <int G>
__global__ __launch_bounds__(256) void cons_compact_kernel(const int32_t *__restrict__ key, const double2 *__restrict__ uv, const int64_t *__restrict__ start,
                                                           const uint8_t *__restrict__ flag, const int64_t *__restrict__ c_start, const int64_t n,
                                                           int32_t *__restrict__ c_key, double2 *__restrict__ c_uv) {
    static_assert(G <= 16 && 64 % G == 0, "a group's bits are cut from the 64-bit ballot of its wave");
    const int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const int g = threadIdx.x & (G - 1);
    if (j >= n) return;
    const int shift = (threadIdx.x & 63) & ~(G - 1);
    const int64_t s0 = start[j], s1 = start[j + 1], end = c_start[j + 1];
    int64_t base = c_start[j];
    for (int64_t c = s0; c < s1; c += G) {   // the trip count is the group's: the lanes of a group stay together
        const int64_t o = c + g;
        const bool f = o < s1 && flag[o] != 0;
        const uint32_t bits = (uint32_t)(__ballot(f) >> shift) & ((1u << G) - 1u);
        const int64_t pos = base + __popc(bits & ((1u << g) - 1u));
        if (f && pos < end) {
            c_key[pos] = key[o];
            c_uv[pos] = uv[o];
        }
        base += __popc(bits);
    }
}

// out[stride j + column] = rows of problem j
__global__ __launch_bounds__(256) void cons_restore_count_kernel(const int64_t *__restrict__ start, const int64_t n, int32_t *__restrict__ out, const int stride,
                                                                 const int column) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    out[(int64_t)stride * j + column] = (int32_t)(start[j + 1] - start[j]);
}

}  // namespace pcs
