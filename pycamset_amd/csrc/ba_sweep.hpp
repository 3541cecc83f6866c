// ba_sweep.hpp — plane-sweep multi-view depth: from the images of a rig to one z-depth map per view (include/pcs_hip.h, "Plane-sweep
// depth"; host side: pcs_sweep.inc).  One launch.  A workgroup of 256 threads owns a TW x (SWEEP_PPT 256 / TW) tile of
// ONE view, so that the view, its neighbour list, the warp of a slot and the plane depth are the same in every lane and come through
// scalar loads; a thread owns SWEEP_PPT pixels of one column of the tile, 256 / TW rows apart.  The cost volume is never stored: the
// workgroup walks the planes k and, inside, the neighbour slots j, and per (k, j)
//   1. stages the warped samples g (uint16, 0xFFFF = invalid) of tile + halo (box radius + census radius on every side) in LDS — the
//      only floating-point step, FP64 with contraction OFF: the rule is a sequence of plain IEEE operations in the order written;
//   2. derives the census descriptor of every cell of tile + box halo from LDS, xors it with the reference descriptor (computed once
//      per workgroup, in LDS) and stores the Hamming distance (uint8, 0xFF = some sample of the window invalid);
//   3. box-sums the distances per pixel, truncates, and adds the slot's cost to the plane's cost in a register.
// Two barriers per (k, j): a stage writes `smp` while the previous box sums still read `ham`, and a census writes `ham` only behind the
// barrier that every box sum of the previous slot has passed.  Behind the slots of plane k each pixel's decision state takes C(k): the
// four smallest (cost, k) entries in a sorted insert — the winner is the first, and the smallest cost at |k - k*| >= 2 is among them
// because at most two entries are adjacent to k* — and the winner's two neighbours for the sub-plane offset.  All of it sits in
// registers under compile-time indices; nothing per lane is indexed at run time.  No atomics; every sum is an integer: two runs, any
// tile and any order of a neighbour list give identical bits.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace pcs {

constexpr int SWEEP_THREADS = 256, SWEEP_PPT = 4;   // pixels per thread: tile = TW x (SWEEP_PPT * 256 / TW)
constexpr int SWEEP_MAX_NBR = 16, SWEEP_MAX_PLANES = 1024, SWEEP_MAX_BOX = 4;
constexpr int SWEEP_BAD_SAMPLE = 0xFFFF;            // g <= 255 * 256 = 65280
constexpr int SWEEP_BAD_HAMMING = 0xFF;             // h <= 64
enum : int { SWEEP_NOT_STRICT = 1, SWEEP_NO_VIEW = 2, SWEEP_UNIQUENESS = 4 };

struct SweepArgs {
    const uint8_t *images;      // (V, H, pitch)
    int64_t pitch;
    const double *warp;         // (entries of nbr, 12): A row-major, then b — the warp of reference view i into its neighbour slot
    const int32_t *nbr_start;   // (V + 1)
    const int32_t *nbr;
    const double *z;            // (n_z, D) plane depths
    int z_stride;               // 0 (one row for all views) or D
    int D, W, H;
    int rw, rh, r;              // census radii and box radius
    int tau, uniq;
    int tw_log2;                // tile width TW = 1 << tw_log2 in [8, 64]
    void *depth;                // (V, H, W) float or double
    int depth_f32;
    int32_t *level, *cost;      // (V, H, W) or NULL
    uint8_t *status;            // (V, H, W) or NULL
};

// bytes of LDS of a workgroup: reference descriptors (8) and distances (1) of tile + box halo, samples (2) of tile + whole halo
__host__ __device__ inline int64_t sweep_lds_bytes(int tw, int rw, int rh, int r) {
    const int64_t th = SWEEP_PPT * SWEEP_THREADS / tw;
    const int64_t cells = (int64_t)(tw + 2 * r) * (th + 2 * r), samples = (int64_t)(tw + 2 * (r + rw)) * (th + 2 * (r + rh));
    return 8 * cells + 2 * samples + ((cells + 7) & ~(int64_t)7);
}

// The warped sample of reference pixel (xd, yd) at plane depth zk in the neighbour image I: steps 1 and 2 of the rule.
__device__ __forceinline__ int sweep_sample(const double *__restrict__ w, double zk, double xd, double yd, const uint8_t *__restrict__ I, int64_t pitch, int W, int H) {
#pragma clang fp contract(off)
    const double n0 = zk * ((w[0] * xd + w[1] * yd) + w[2]) + w[9];
    const double n1 = zk * ((w[3] * xd + w[4] * yd) + w[5]) + w[10];
    const double n2 = zk * ((w[6] * xd + w[7] * yd) + w[8]) + w[11];
    if (!(n2 > 0.0)) return SWEEP_BAD_SAMPLE;
    const double u = n0 / n2, v = n1 / n2;
    const double qu = floor(16.0 * u + 0.5), qv = floor(16.0 * v + 0.5);
    if (!(qu >= 0.0 && qu < 16.0 * (double)(W - 1) && qv >= 0.0 && qv < 16.0 * (double)(H - 1))) return SWEEP_BAD_SAMPLE;   // a NaN fails
    const int iu = (int)qu, iv = (int)qv;   // converted only once known to lie inside
    const int x0 = iu >> 4, fx = iu & 15, y0 = iv >> 4, fy = iv & 15;
    const uint8_t *__restrict__ p = I + (int64_t)y0 * pitch + x0;   // x0 + 1 <= W - 1 and y0 + 1 <= H - 1
    return (16 - fx) * (16 - fy) * (int)p[0] + fx * (16 - fy) * (int)p[1] + (16 - fx) * fy * (int)p[pitch] + fx * fy * (int)p[pitch + 1];
}

// The decision state of one pixel: the four smallest (cost, k), sorted, ties to the lower k; the cost of the previous plane; the costs
// of the planes in front of and behind the winner.
struct SweepState {
    int c0, c1, c2, c3, k0, k1, k2, k3, prev, m, p;
};

__device__ __forceinline__ void sweep_take(SweepState &s, int C, int k) {
    if (k == s.k0 + 1) s.p = C;
    if (C < s.c0) s.m = s.prev;   // k becomes the winner
    s.prev = C;
    // the sorted insert, from the back: planes arrive in rising k, so an equal cost goes BEHIND the entries that hold it
    const bool b3 = C < s.c3, b2 = C < s.c2, b1 = C < s.c1, b0 = C < s.c0;
    s.c3 = b2 ? s.c2 : b3 ? C : s.c3, s.k3 = b2 ? s.k2 : b3 ? k : s.k3;
    s.c2 = b1 ? s.c1 : b2 ? C : s.c2, s.k2 = b1 ? s.k1 : b2 ? k : s.k2;
    s.c1 = b0 ? s.c0 : b1 ? C : s.c1, s.k1 = b0 ? s.k0 : b1 ? k : s.k1;
    s.c0 = b0 ? C : s.c0, s.k0 = b0 ? k : s.k0;
}

__global__ __launch_bounds__(SWEEP_THREADS) void sweep_kernel(const SweepArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char sweep_lds[];
    const int i = blockIdx.z, tid = threadIdx.x;
    const int W = a.W, H = a.H, rw = a.rw, rh = a.rh, r = a.r;
    const int TW = 1 << a.tw_log2, TR = SWEEP_THREADS >> a.tw_log2, TH = SWEEP_PPT * TR;   // TR: rows between a thread's pixels
    const int BW = TW + 2 * r, BH = TH + 2 * r, cells = BW * BH;                            // tile + box halo
    const int SW = BW + 2 * rw, SH = BH + 2 * rh, samples = SW * SH;                        // tile + box halo + census halo
    uint64_t *ref = reinterpret_cast<uint64_t *>(sweep_lds);
    uint16_t *smp = reinterpret_cast<uint16_t *>(ref + cells);
    uint8_t *ham = reinterpret_cast<uint8_t *>(smp + samples);
    const int tx = tid & (TW - 1), ty = tid >> a.tw_log2;
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, x = tx0 + tx;
    // the strict rectangle, ends inclusive
    const int xs0 = rw + r, xs1 = W - 1 - rw - r, ys0 = rh + r, ys1 = H - 1 - rh - r;
    const int64_t HW = (int64_t)H * W;
    const int n0 = a.nbr_start[i], len = a.nbr_start[i + 1] - n0;
    const bool any_strict = max(tx0, xs0) <= min(tx0 + TW - 1, xs1) && max(ty0, ys0) <= min(ty0 + TH - 1, ys1);   // the same in every lane

    SweepState st[SWEEP_PPT];
#pragma unroll
    for (int q = 0; q < SWEEP_PPT; ++q) {
        st[q].c0 = st[q].c1 = st[q].c2 = st[q].c3 = INT_MAX;
        st[q].k0 = st[q].k1 = st[q].k2 = st[q].k3 = -2;
        st[q].prev = st[q].m = st[q].p = 0;
    }

    if (any_strict) {
        const uint8_t *__restrict__ Ii = a.images + (int64_t)i * H * a.pitch;
        if (len > 0)   // the reference descriptors of tile + box halo; 0 where the window leaves the image (no strict pixel reads those)
            for (int c = tid; c < cells; c += SWEEP_THREADS) {
                const int by = c / BW, bx = c - by * BW, px = tx0 - r + bx, py = ty0 - r + by;
                uint64_t bits = 0;
                if (px - rw >= 0 && px + rw < W && py - rh >= 0 && py + rh < H) {
                    const uint8_t *__restrict__ p = Ii + (int64_t)py * a.pitch + px;
                    const int centre = p[0];
                    for (int dy = -rh; dy <= rh; ++dy)
                        for (int dx = -rw; dx <= rw; ++dx)
                            if (dx != 0 || dy != 0) bits = (bits << 1) | (uint64_t)((int)p[(int64_t)dy * a.pitch + dx] < centre);
                }
                ref[c] = bits;
            }
        const double *__restrict__ zrow = a.z + (int64_t)i * a.z_stride;
        for (int k = 0; k < a.D; ++k) {
            const double zk = zrow[k];
            int C[SWEEP_PPT];
#pragma unroll
            for (int q = 0; q < SWEEP_PPT; ++q) C[q] = 0;
            for (int s = 0; s < len; ++s) {   // the same trip count and the same neighbour in every lane
                const int j = a.nbr[n0 + s];
                const double *__restrict__ w = a.warp + 12 * (int64_t)(n0 + s);
                const uint8_t *__restrict__ Ij = a.images + (int64_t)j * H * a.pitch;
                for (int c = tid; c < samples; c += SWEEP_THREADS) {
                    const int sy = c / SW, sx = c - sy * SW, px = tx0 - r - rw + sx, py = ty0 - r - rh + sy;
                    int g = SWEEP_BAD_SAMPLE;
                    if (px >= 0 && px < W && py >= 0 && py < H) g = sweep_sample(w, zk, (double)px, (double)py, Ij, a.pitch, W, H);
                    smp[c] = (uint16_t)g;
                }
                __syncthreads();
                for (int c = tid; c < cells; c += SWEEP_THREADS) {
                    const int by = c / BW, bx = c - by * BW;
                    const uint16_t *__restrict__ row = smp + (by + rh) * SW + bx + rw;
                    const int centre = row[0];
                    bool ok = centre != SWEEP_BAD_SAMPLE;
                    uint64_t bits = 0;
                    for (int dy = -rh; dy <= rh; ++dy)
                        for (int dx = -rw; dx <= rw; ++dx)
                            if (dx != 0 || dy != 0) {
                                const int v = row[dy * SW + dx];
                                ok = ok && v != SWEEP_BAD_SAMPLE;
                                bits = (bits << 1) | (uint64_t)(v < centre);
                            }
                    ham[c] = (uint8_t)(ok ? __popcll(bits ^ ref[c]) : SWEEP_BAD_HAMMING);
                }
                __syncthreads();
#pragma unroll
                for (int q = 0; q < SWEEP_PPT; ++q) {
                    const uint8_t *__restrict__ h0 = ham + (ty + q * TR) * BW + tx;
                    int sum = 0;
                    bool ok = true;
                    for (int dy = 0; dy <= 2 * r; ++dy)
                        for (int dx = 0; dx <= 2 * r; ++dx) {
                            const int h = h0[dy * BW + dx];
                            ok = ok && h != SWEEP_BAD_HAMMING;
                            sum += h;
                        }
                    C[q] += ok && sum < a.tau ? sum : a.tau;
                }
            }
#pragma unroll
            for (int q = 0; q < SWEEP_PPT; ++q) sweep_take(st[q], C[q], k);
        }
    }

    const double *__restrict__ zrow = a.z + (int64_t)i * a.z_stride;
#pragma unroll
    for (int q = 0; q < SWEEP_PPT; ++q) {
        const int y = ty0 + ty + q * TR;
        if (x >= W || y >= H) continue;
        const int64_t g = (int64_t)i * HW + (int64_t)y * W + x;
        const bool strict = x >= xs0 && x <= xs1 && y >= ys0 && y <= ys1;
        const SweepState s = st[q];
        int status = SWEEP_NOT_STRICT, level = -16, cost = -1;
        double depth = __builtin_nan("");
        if (strict) {
            const int ks = s.k0, Cs = s.c0;
            int f = 0;
            if (ks > 0 && ks < a.D - 1) {
                const int den = 2 * (s.m + s.p - 2 * Cs);   // > 0: the plane in front of the first minimum costs more
                if (den != 0) {
                    const int num = 32 * (s.m - s.p) + den;   // floor division
                    f = num >= 0 ? num / (2 * den) : -((-num + 2 * den - 1) / (2 * den));
                }
            }
            // the smallest cost at |k - k*| >= 2: the first such entry behind the winner
            int far = INT_MAX;
            if (s.k3 >= 0 && abs(s.k3 - ks) >= 2) far = s.c3;
            if (s.k2 >= 0 && abs(s.k2 - ks) >= 2) far = s.c2;
            if (s.k1 >= 0 && abs(s.k1 - ks) >= 2) far = s.c1;
            status = Cs >= a.tau * len ? SWEEP_NO_VIEW : (a.uniq > 0 && far != INT_MAX && 100 * (int64_t)far <= (int64_t)(100 + a.uniq) * Cs) ? SWEEP_UNIQUENESS : 0;
            level = 16 * ks + f, cost = Cs;
            if (status == 0) {
                const double zs = zrow[ks], zn = zrow[ks + (f > 0 ? 1 : f < 0 ? -1 : 0)];
                depth = zs + ((double)abs(f) / 16.0) * (zn - zs);
            }
        }
        if (a.depth_f32) static_cast<float *>(a.depth)[g] = (float)depth;
        else static_cast<double *>(a.depth)[g] = depth;
        if (a.level) a.level[g] = level;
        if (a.cost) a.cost[g] = cost;
        if (a.status) a.status[g] = (uint8_t)status;
    }
}

}  // namespace pcs
