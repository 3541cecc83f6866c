// ba_groupstats.hpp — per-group statistics of a residual vector that already sits in device memory.
//
// After a solve the reference judges the result on the host: the per-image error of template_handler.py:535-560 goes through the MAD test
// of utils/general_utils.py:108-133 (template_handler.py:242-279), optimisation_handling.py:66-70 prints one mean.  Here every
// detection's error e = |(ru, rv)| and, per camera, per image, per key, per view = (camera, image) and over all rows, the count, the sums
// that give mean / RMS / bias, the worst detection and the exact median and MAD are made on the device from the residual buffer.
//
// The groups of all five groupings share ONE index space ("flat groups"): camera c is group c, image i is C + i, key k is C + I + k, view
// (c, i) is C + I + K + c I + i, and the single group over all rows is the last one, C + I + K + C I.
//
// Index (once per table): gs_keys_kernel writes, per grouping, the flat group of every row (4 n keys, grouping-major, rows ascending) and
//   range-checks the ids (the lowest bad row through an INTEGER atomicMin).  An LSD radix sort by 8-bit digits orders the 4 n (key, row)
//   pairs by flat group: gs_sort_hist_kernel counts the digits of every chunk of GS_SORT_CHUNK pairs (LDS integer atomics: counts do not
//   depend on arrival order), gs_scan_kernel turns the (digit, chunk) counts into offsets, gs_sort_scatter_kernel — one wave per chunk —
//   walks its chunk 64 pairs at a time and ranks every pair among the lanes of equal digit with ballots.  Every pass is stable, so the
//   rows of a group end up in ASCENDING TABLE ORDER whatever the order of the table.  gs_starts_kernel reads the group boundaries off the
//   sorted keys (empty groups included); the fifth grouping is the identity permutation behind the four sorted ones.
// Run: gs_error_kernel e[i] = sqrt(ru^2 + rv^2), every operation rounded on its own (no contraction); gs_gather_kernel lays e out in
//   group order, so that the passes below read each group's errors side by side; gs_stats_kernel, one workgroup per flat group, the
//   largest groups first (enqueue_group_order, walked backwards): thread t owns the group's rows t, t + 256, ... in ascending order, the
//   sums go through fixed trees (64-lane xor shuffles, then the four waves in order through LDS), the worst detection ties to the lowest
//   row.  There are no floating-point atomics: two runs give the same bits.
//   A detection whose e is not finite is counted in n_nonfinite and takes no part in anything else.
//   Median and MAD are exact order statistics by radix selection on the bit pattern: e >= 0, so the unsigned order of its bits is its
//   numeric order.  Eight passes of 8 bits, most significant first; a pass counts, in an LDS histogram (integer atomics), the next digit
//   of the values that share the digits found so far, and wave 0 finds the digit that holds rank k.  For an even count a ninth pass finds
//   the next order statistic (the same value when it repeats, else the smallest larger one).  Nothing is stored per group, so a group of
//   any size is selected in place; the MAD runs the same selection over |e - median|.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcs {

constexpr int GS_GROUPINGS = 5;
constexpr int GS_SORT_CHUNK = 2048;   // pairs per wave of a sort pass
constexpr int GS_THREADS = 256;       // threads of a statistics workgroup
constexpr int GS_UNROLL = 4;          // independent loads per thread and stride of a selection pass (counts and minima: any order)
constexpr int GS_INTS = 3;            // count, n_nonfinite, argmax
constexpr int GS_VALS = 7;            // sum_e, sum_e2, sum_ru, sum_rv, max_e, median, mad
constexpr int GS_NO_ORDER_STATISTICS = 1;

// ---- index ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gs_keys_kernel(const int32_t *__restrict__ cam, const int32_t *__restrict__ img, const int32_t *__restrict__ key,
                                                      const int64_t n, const int32_t C, const int32_t I, const int32_t K, int32_t *__restrict__ keys,
                                                      int32_t *__restrict__ rows, int32_t *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t c = cam[i], im = img[i], k = key[i];
    if (c < 0 || c >= C || im < 0 || im >= I || k < 0 || k >= K) {
        atomicMin(bad, (int32_t)i);   // the build is refused; the keys below only have to stay inside the index space
        c = im = k = 0;
    }
    keys[i] = c;
    keys[n + i] = C + im;
    keys[2 * n + i] = C + I + k;
    keys[3 * n + i] = C + I + K + c * I + im;
#pragma unroll
    for (int g = 0; g < 4; ++g) rows[g * n + i] = (int32_t)i;
}

__global__ __launch_bounds__(64) void gs_sort_hist_kernel(const int32_t *__restrict__ keys, const int64_t m, const int shift, int32_t *__restrict__ blockhist,
                                                          const int64_t n_chunks) {
    __shared__ int32_t h[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += 64) h[d] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * GS_SORT_CHUNK, hi = lo + GS_SORT_CHUNK < m ? lo + GS_SORT_CHUNK : m;
    for (int64_t i = lo + lane; i < hi; i += 64) atomicAdd(&h[(keys[i] >> shift) & 255], 1);
    __syncthreads();
    for (int d = lane; d < 256; d += 64) blockhist[(int64_t)d * n_chunks + blockIdx.x] = h[d];   // digit-major: one scan gives every chunk's offsets
}

// exclusive scan of `len` int32 in place, one workgroup of 1024 threads: thread t owns a contiguous span
__global__ __launch_bounds__(1024) void gs_scan_kernel(int32_t *__restrict__ data, const int64_t len) {
    __shared__ int32_t sm[1024];
    const int t = threadIdx.x;
    const int64_t span = (len + 1023) / 1024, lo = span * t < len ? span * t : len, hi = lo + span < len ? lo + span : len;
    int32_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += data[i];
    sm[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int32_t add = t >= off ? sm[t - off] : 0;
        __syncthreads();
        sm[t] += add;
        __syncthreads();
    }
    int32_t acc = sm[t] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        const int32_t v = data[i];
        data[i] = acc;
        acc += v;
    }
}

__global__ __launch_bounds__(64) void gs_sort_scatter_kernel(const int32_t *__restrict__ keys_in, const int32_t *__restrict__ rows_in, const int64_t m, const int shift,
                                                             const int32_t *__restrict__ offsets, const int64_t n_chunks, int32_t *__restrict__ keys_out,
                                                             int32_t *__restrict__ rows_out) {
    __shared__ int32_t cursor[256];
    const int lane = threadIdx.x;
    for (int d = lane; d < 256; d += 64) cursor[d] = offsets[(int64_t)d * n_chunks + blockIdx.x];
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * GS_SORT_CHUNK, hi = lo + GS_SORT_CHUNK < m ? lo + GS_SORT_CHUNK : m;
    for (int64_t base = lo; base < hi; base += 64) {   // uniform trip count: the ballots below need every lane
        const int64_t i = base + lane;
        const bool valid = i < hi;
        const int32_t kv = valid ? keys_in[i] : 0, rv = valid ? rows_in[i] : 0;
        const int d = (kv >> shift) & 255;
        unsigned long long same = __ballot(valid);   // the valid lanes of equal digit
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1;
            const unsigned long long with = __ballot(valid && bit);
            same &= bit ? with : ~with;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        const int32_t pos = valid ? cursor[d] + rank : 0;
        __syncthreads();
        if (valid && rank == 0) cursor[d] += __popcll(same);   // one lane per digit
        __syncthreads();
        if (valid) {
            keys_out[pos] = kv;
            rows_out[pos] = rv;
        }
    }
}

// start[q] = first position of flat group q among the m sorted keys, for q = 0 .. n_sorted_groups (the end of the last one); the
// single group over all rows follows: start[n_sorted_groups + 1] = m + n.
__global__ __launch_bounds__(256) void gs_starts_kernel(const int32_t *__restrict__ keys, const int64_t m, const int64_t n, const int32_t n_sorted_groups,
                                                        int64_t *__restrict__ start) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > m) return;
    const int32_t prev = i == 0 ? -1 : keys[i - 1], cur = i == m ? n_sorted_groups : keys[i];
    for (int32_t q = prev + 1; q <= cur; ++q) start[q] = i;
    if (i == m) start[n_sorted_groups + 1] = m + n;
}

__global__ __launch_bounds__(256) void gs_iota_kernel(int32_t *__restrict__ out, const int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (int32_t)i;
}

// ---- run -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gs_error_kernel(const double *__restrict__ resid, const int64_t n, double *__restrict__ e) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double ru = resid[2 * i], rv = resid[2 * i + 1];
    const double uu = ru * ru, vv = rv * rv;
    e[i] = sqrt(uu + vv);   // two squares, one sum, one root, each rounded on its own
}

__global__ __launch_bounds__(256) void gs_gather_kernel(const double *__restrict__ e, const int32_t *__restrict__ perm, const int64_t m, double *__restrict__ eg) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < m) eg[p] = e[perm[p]];
}

__device__ __forceinline__ bool gs_finite_bits(const unsigned long long b) { return (b & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// the value a selection ranks: e itself, or its distance from the median
template <bool DEV> __device__ __forceinline__ unsigned long long gs_rank_bits(const double ev, const double med) {
    return (unsigned long long)__double_as_longlong(DEV ? fabs(ev - med) : ev);
}

struct GsShared {
    int32_t hist[256];
    double d[4][GS_THREADS / 64];
    int32_t i[3][GS_THREADS / 64];
    unsigned long long u[GS_THREADS / 64];
    unsigned long long prefix;
    int64_t k;
};

// sum over the workgroup, the same value in every thread: xor shuffles inside a wave, then the waves in order
__device__ __forceinline__ double gs_wave_sum(double x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
__device__ __forceinline__ int32_t gs_wave_sum(int32_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// Bits of the k-th smallest (k from 0) of the group's ranked values, and in *next those of the (k + 1)-th when want_next.  Every thread
// of the workgroup calls it with the same arguments and gets the same result.  0 <= k < number of finite rows (k + 1 < when want_next).
template <bool DEV>
__device__ unsigned long long gs_select(const double *__restrict__ eg, const int64_t s0, const int64_t s1, const double med, const int64_t k, const bool want_next,
                                        unsigned long long *next, GsShared &sm) {
    const int t = threadIdx.x;
    unsigned long long prefix = 0;
    int64_t kk = k;
    for (int pass = 7; pass >= 0; --pass) {
        const int shift = 8 * pass;
        sm.hist[t] = 0;   // GS_THREADS == 256 bins
        __syncthreads();
        for (int64_t p0 = s0 + t; p0 < s1; p0 += GS_UNROLL * GS_THREADS) {   // GS_UNROLL loads in flight: a long group is bound by their latency
            double ev[GS_UNROLL];
#pragma unroll
            for (int j = 0; j < GS_UNROLL; ++j) ev[j] = p0 + j * GS_THREADS < s1 ? eg[p0 + j * GS_THREADS] : __builtin_nan("");
#pragma unroll
            for (int j = 0; j < GS_UNROLL; ++j) {
                if (!gs_finite_bits((unsigned long long)__double_as_longlong(ev[j]))) continue;
                const unsigned long long v = gs_rank_bits<DEV>(ev[j], med);
                if (pass == 7 || (v >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sm.hist[(int)((v >> shift) & 255)], 1);
            }
        }
        __syncthreads();
        if (t < 64) {   // wave 0: lane l owns bins 4 l .. 4 l + 3; the bin that holds rank kk
            const int32_t c0 = sm.hist[4 * t], c1 = sm.hist[4 * t + 1], c2 = sm.hist[4 * t + 2], c3 = sm.hist[4 * t + 3];
            int64_t incl = (int64_t)c0 + c1 + c2 + c3;
            const int64_t own = incl;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int64_t up = __shfl_up(incl, off);
                if (t >= off) incl += up;
            }
            int64_t excl = incl - own;
            if (kk >= excl && kk < incl) {   // exactly one lane
                int digit = 4 * t;
                if (kk >= excl + c0) { excl += c0, ++digit;
                    if (kk >= excl + c1) { excl += c1, ++digit;
                        if (kk >= excl + c2) { excl += c2, ++digit; } } }
                sm.prefix = prefix | ((unsigned long long)digit << shift);
                sm.k = kk - excl;
            }
        }
        __syncthreads();
        prefix = sm.prefix;
        kk = sm.k;
    }
    if (want_next) {   // how many values do not exceed the one found, and the smallest that does
        int32_t le = 0;
        unsigned long long above = ~0ull;
        for (int64_t p0 = s0 + t; p0 < s1; p0 += GS_UNROLL * GS_THREADS) {
            double ev[GS_UNROLL];
#pragma unroll
            for (int j = 0; j < GS_UNROLL; ++j) ev[j] = p0 + j * GS_THREADS < s1 ? eg[p0 + j * GS_THREADS] : __builtin_nan("");
#pragma unroll
            for (int j = 0; j < GS_UNROLL; ++j) {
                if (!gs_finite_bits((unsigned long long)__double_as_longlong(ev[j]))) continue;
                const unsigned long long v = gs_rank_bits<DEV>(ev[j], med);
                if (v <= prefix) ++le;
                else if (v < above) above = v;
            }
        }
        le = gs_wave_sum(le);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(above, off);
            above = o < above ? o : above;
        }
        __syncthreads();   // sm.i / sm.u may still be read from an earlier reduction
        if ((t & 63) == 0) sm.i[0][t >> 6] = le, sm.u[t >> 6] = above;
        __syncthreads();
        int64_t n_le = 0;
        unsigned long long mn = ~0ull;
#pragma unroll
        for (int w = 0; w < GS_THREADS / 64; ++w) {
            n_le += sm.i[0][w];
            mn = sm.u[w] < mn ? sm.u[w] : mn;
        }
        *next = n_le >= k + 2 ? prefix : mn;
    }
    return prefix;
}

template <bool DEV>
__device__ double gs_median(const double *__restrict__ eg, const int64_t s0, const int64_t s1, const double med, const int64_t n, GsShared &sm) {
#pragma clang fp contract(off)
    unsigned long long b = 0;
    if (n & 1) return __longlong_as_double((long long)gs_select<DEV>(eg, s0, s1, med, (n - 1) / 2, false, &b, sm));
    const unsigned long long a = gs_select<DEV>(eg, s0, s1, med, n / 2 - 1, true, &b, sm);
    return (__longlong_as_double((long long)a) + __longlong_as_double((long long)b)) * 0.5;
}

// One workgroup per flat group.  ints: (GS_INTS, n_groups) = count, n_nonfinite, argmax; vals: (GS_VALS, n_groups) = sum_e, sum_e2,
// sum_ru, sum_rv, max_e, median, mad.
__global__ __launch_bounds__(GS_THREADS) void gs_stats_kernel(const double *__restrict__ resid, const double *__restrict__ eg, const int32_t *__restrict__ perm,
                                                              const int64_t *__restrict__ start, const int32_t *__restrict__ order, const int64_t n_groups,
                                                              const int flags, int32_t *__restrict__ ints, double *__restrict__ vals) {
#pragma clang fp contract(off)
    __shared__ GsShared sm;
    const int t = threadIdx.x, w = t >> 6;
    const int64_t q = order[n_groups - 1 - blockIdx.x];   // the largest groups first
    const int64_t s0 = start[q], s1 = start[q + 1];
    double se = 0.0, se2 = 0.0, su = 0.0, sv = 0.0, mx = 0.0;
    int32_t cnt = 0, bad = 0, arg = -1;
    for (int64_t p = s0 + t; p < s1; p += GS_THREADS) {
        const double ev = eg[p];
        if (!gs_finite_bits((unsigned long long)__double_as_longlong(ev))) {
            ++bad;
            continue;
        }
        const int32_t row = perm[p];
        ++cnt;
        const double ee = ev * ev;
        se += ev;
        se2 += ee;
        su += resid[2 * (int64_t)row];
        sv += resid[2 * (int64_t)row + 1];
        if (arg < 0 || ev > mx) mx = ev, arg = row;   // rows ascend along p: the first of equal maxima is the lowest row
    }
    se = gs_wave_sum(se), se2 = gs_wave_sum(se2), su = gs_wave_sum(su), sv = gs_wave_sum(sv);
    cnt = gs_wave_sum(cnt), bad = gs_wave_sum(bad);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double omx = __shfl_xor(mx, off);
        const int32_t oarg = __shfl_xor(arg, off);
        if (oarg >= 0 && (arg < 0 || omx > mx || (omx == mx && oarg < arg))) mx = omx, arg = oarg;
    }
    if ((t & 63) == 0) {
        sm.d[0][w] = se, sm.d[1][w] = se2, sm.d[2][w] = su, sm.d[3][w] = sv;
        sm.i[0][w] = cnt, sm.i[1][w] = bad, sm.i[2][w] = arg;
        sm.u[w] = (unsigned long long)__double_as_longlong(mx);
    }
    __syncthreads();
    static_assert(GS_THREADS == 256, "four waves: the trees below and the 256 bins of the selection");
    se = (sm.d[0][0] + sm.d[0][1]) + (sm.d[0][2] + sm.d[0][3]);
    se2 = (sm.d[1][0] + sm.d[1][1]) + (sm.d[1][2] + sm.d[1][3]);
    su = (sm.d[2][0] + sm.d[2][1]) + (sm.d[2][2] + sm.d[2][3]);
    sv = (sm.d[3][0] + sm.d[3][1]) + (sm.d[3][2] + sm.d[3][3]);
    int64_t n = 0;
    int32_t n_bad = 0;
    arg = -1, mx = 0.0;
#pragma unroll
    for (int k = 0; k < GS_THREADS / 64; ++k) {
        n += sm.i[0][k];
        n_bad += sm.i[1][k];
        const int32_t oarg = sm.i[2][k];
        const double omx = __longlong_as_double((long long)sm.u[k]);
        if (oarg >= 0 && (arg < 0 || omx > mx || (omx == mx && oarg < arg))) mx = omx, arg = oarg;
    }
    const double qnan = __builtin_nan("");
    double med = qnan, mad = qnan;
    if (n > 0 && !(flags & GS_NO_ORDER_STATISTICS)) {   // n is uniform over the workgroup
        med = gs_median<false>(eg, s0, s1, 0.0, n, sm);
        mad = gs_median<true>(eg, s0, s1, med, n, sm);
    }
    if (t == 0) {
        ints[q] = (int32_t)n;
        ints[n_groups + q] = n_bad;
        ints[2 * n_groups + q] = arg;
        vals[q] = se;
        vals[n_groups + q] = se2;
        vals[2 * n_groups + q] = su;
        vals[3 * n_groups + q] = sv;
        vals[4 * n_groups + q] = n > 0 ? mx : qnan;
        vals[5 * n_groups + q] = med;
        vals[6 * n_groups + q] = mad;
    }
}

}  // namespace pcs
