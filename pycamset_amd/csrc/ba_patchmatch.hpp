// ba_patchmatch.hpp — PatchMatch multi-view depth: one slanted plane (w, a, b) per pixel of every view, spread between neighbouring
// pixels and refined by random perturbation (include/pcs_hip.h, "PatchMatch multi-view depth"; host side:
// pcs_patchmatch.inc).  Three kernels: pm_init_kernel (t = 0: start planes and their costs), pm_half_kernel (one colour of the
// checkerboard: 8 propagated and 4 perturbed candidates per pixel) and pm_finish_kernel (status, depth, normal).
// A workgroup of 256 threads of pm_half_kernel owns a TW x (512 / TW) tile of ONE view, so that the view, its neighbour list and the
// 12 numbers of a slot's warp are the same in every lane and come through scalar loads.  Only the pixels of the launch's colour are
// active, so they are packed densely: lane t owns pixel (2 k + ((c + y) & 1), t / (TW / 2)) of the tile, k = t % (TW / 2) — no lane
// idles for the other colour.  The other colour's planes are read where they stand: a launch writes pixels of its own colour only, so
// they are the state before the half-iteration for every tile and every order of the workgroups; they are read 8 times per pixel
// against 12 x (list length) x cw ch warped samples of four byte gathers each, and stay in the caches.  Unlike the sweep, nothing can
// be staged per tile: a sample's position depends on the lane's own plane.  The reference descriptor of a pixel is computed once, by
// its own lane (no box joins pixels here), and lives in two registers.  A candidate's cost is an integer; the only floating-point
// steps are the plane arithmetic and the warp, FP64 with contraction OFF: plain IEEE operations in the order the header writes.
// All per-lane state sits in scalars; nothing is indexed at run time.  No atomics: two runs, any tile and any order of a neighbour
// list give identical bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_consensus.hpp"
#include "ba_sweep.hpp"

namespace pcs {

constexpr int PM_THREADS = 256, PM_TILE_PIXELS = 512;   // a tile holds 256 pixels of either colour
constexpr int PM_MAX_NBR = 16, PM_MAX_STRIDE = 4, PM_MAX_ITERATION = 1000;   // 2^-(2 + it) stays a normal double
enum : int { PM_NOT_STRICT = 1, PM_NO_VIEW = 2 };
constexpr int PM_VIEW_WORDS = 8;   // per view: w_lo, w_hi, sigma, fx, cx, fy, cy, unused

struct PmArgs {
    const uint8_t *images;      // (V, H, pitch)
    int64_t pitch;
    const double *warp;         // (entries of nbr, 12): the sweep's table
    const int32_t *nbr_start;   // (V + 1)
    const int32_t *nbr;
    const double *view;         // (V, PM_VIEW_WORDS)
    int W, H;
    int rw, rh, stride, tau;
    uint64_t seed;
    double *plane;              // (V, H, W, 3)
    int32_t *cost;              // (V, H, W)
    // pm_init_kernel
    const void *start_depth;    // (V, H, W) float or double, or NULL
    int start_f32, start_planes;
    // pm_half_kernel
    int it, colour, tw_log2;
    double rho, half_it;        // 2^-(2 + it) and 2^-(1 + it), formed on the host: both scalings are exact
    // pm_finish_kernel
    void *depth, *normal;       // (V, H, W) and (V, H, W, 3), float or double; normal may be NULL
    int out_f32;
    uint8_t *status;            // (V, H, W) or NULL
};

struct PmPlane {
    double w, a, b;
};

__device__ __forceinline__ uint64_t pm_key(uint64_t seed, int view, int64_t pixel, int t) {
    uint64_t k = cons_mix64(seed + CONS_GOLDEN);
    k = cons_mix64(k ^ (uint64_t)view);
    k = cons_mix64(k ^ (uint64_t)pixel);
    return cons_mix64(k ^ (uint64_t)t);
}

__device__ __forceinline__ double pm_rand(uint64_t k, int d) {   // exact, in [0, 1)
    return (double)(cons_mix64(k + (uint64_t)(d + 1) * CONS_GOLDEN) >> 11) * 0x1p-53;
}

__device__ __forceinline__ bool pm_strict(const PmArgs &a, int x, int y) {
    return x >= a.rw * a.stride && x <= a.W - 1 - a.rw * a.stride && y >= a.rh * a.stride && y <= a.H - 1 - a.rh * a.stride;
}

__device__ __forceinline__ bool pm_admissible(const PmPlane &p, double w_lo, double w_hi, double sigma) {
#pragma clang fp contract(off)
    const double s = sigma * p.w;
    return p.w >= w_lo && p.w <= w_hi && fabs(p.a) <= s && fabs(p.b) <= s;   // a comparison with a NaN fails
}

// a fresh draw from r_d, r_{d + 1}, r_{d + 2}
__device__ __forceinline__ PmPlane pm_draw(uint64_t k, int d, double w_lo, double w_hi, double sigma) {
#pragma clang fp contract(off)
    PmPlane p;
    p.w = w_lo + pm_rand(k, d) * (w_hi - w_lo);
    const double s = sigma * p.w;
    p.a = s * (2.0 * pm_rand(k, d + 1) - 1.0);
    p.b = s * (2.0 * pm_rand(k, d + 2) - 1.0);
    return p;
}

// The warped sample of reference pixel (xp, yp) at inverse depth om in the neighbour image I: steps 2 and 3 of the rule.
__device__ __forceinline__ int pm_sample(const double *__restrict__ w, double om, int xp, int yp, const uint8_t *__restrict__ I, int64_t pitch, int W, int H) {
#pragma clang fp contract(off)
    const double xd = (double)xp, yd = (double)yp;
    const double n0 = ((w[0] * xd + w[1] * yd) + w[2]) + om * w[9];
    const double n1 = ((w[3] * xd + w[4] * yd) + w[5]) + om * w[10];
    const double n2 = ((w[6] * xd + w[7] * yd) + w[8]) + om * w[11];
    if (!(om > 0.0) || !(n2 > 0.0)) return SWEEP_BAD_SAMPLE;
    const double u = n0 / n2, v = n1 / n2;
    const double qu = floor(16.0 * u + 0.5), qv = floor(16.0 * v + 0.5);
    if (!(qu >= 0.0 && qu < 16.0 * (double)(W - 1) && qv >= 0.0 && qv < 16.0 * (double)(H - 1))) return SWEEP_BAD_SAMPLE;   // a NaN fails
    const int iu = (int)qu, iv = (int)qv;   // converted only once known to lie inside
    const int x0 = iu >> 4, fx = iu & 15, y0 = iv >> 4, fy = iv & 15;
    const uint8_t *__restrict__ p = I + (int64_t)y0 * pitch + x0;   // x0 + 1 <= W - 1 and y0 + 1 <= H - 1
    return (16 - fx) * (16 - fy) * (int)p[0] + fx * (16 - fy) * (int)p[1] + (16 - fx) * fy * (int)p[pitch] + fx * fy * (int)p[pitch + 1];
}

// the census of I_i at the strided positions about the STRICT pixel (x, y): one bit per position other than the centre, rows first
__device__ __forceinline__ uint64_t pm_reference_bits(const PmArgs &a, int i, int x, int y) {
    const uint8_t *__restrict__ p = a.images + (int64_t)i * a.H * a.pitch + (int64_t)y * a.pitch + x;
    const int centre = p[0];
    uint64_t bits = 0;
    for (int dy = -a.rh; dy <= a.rh; ++dy)
        for (int dx = -a.rw; dx <= a.rw; ++dx)
            if (dx != 0 || dy != 0) bits = (bits << 1) | (uint64_t)((int)p[(int64_t)(a.stride * dy) * a.pitch + a.stride * dx] < centre);
    return bits;
}

// C of plane p at strict pixel (x, y) of view i, whose list is entries n0 .. n0 + len of nbr (the same in every lane)
__device__ __forceinline__ int pm_cost(const PmArgs &a, int n0, int len, int x, int y, uint64_t ref, const PmPlane &p) {
#pragma clang fp contract(off)
    int C = 0;
    for (int s = 0; s < len; ++s) {
        const int j = a.nbr[n0 + s];
        const double *__restrict__ w = a.warp + 12 * (int64_t)(n0 + s);
        const uint8_t *__restrict__ Ij = a.images + (int64_t)j * a.H * a.pitch;
        const int centre = pm_sample(w, (p.w + p.a * 0.0) + p.b * 0.0, x, y, Ij, a.pitch, a.W, a.H);
        bool ok = centre != SWEEP_BAD_SAMPLE;
        uint64_t bits = 0;
        for (int dy = -a.rh; dy <= a.rh; ++dy)
            for (int dx = -a.rw; dx <= a.rw; ++dx)
                if ((dx != 0 || dy != 0) && ok) {   // behind the first invalid sample the descriptor is invalid whatever follows
                    const int sx = a.stride * dx, sy = a.stride * dy;
                    const double om = (p.w + p.a * (double)sx) + p.b * (double)sy;
                    const int g = pm_sample(w, om, x + sx, y + sy, Ij, a.pitch, a.W, a.H);
                    ok = g != SWEEP_BAD_SAMPLE;
                    bits = (bits << 1) | (uint64_t)(g < centre);
                }
        const int h = __popcll(bits ^ ref);
        C += ok && h < a.tau ? h : a.tau;
    }
    return C;
}

// t = 0: one thread per pixel of every view
__global__ __launch_bounds__(PM_THREADS) void pm_init_kernel(const PmArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.z, x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const int64_t pix = (int64_t)y * a.W + x, g = (int64_t)i * a.H * a.W + pix;
    PmPlane p{__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    int cost = -1;
    if (pm_strict(a, x, y)) {
        const double *__restrict__ vw = a.view + (int64_t)i * PM_VIEW_WORDS;
        const double w_lo = vw[0], w_hi = vw[1], sigma = vw[2];
        bool have = false;
        if (a.start_planes) {
            p = PmPlane{a.plane[3 * g], a.plane[3 * g + 1], a.plane[3 * g + 2]};
            have = pm_admissible(p, w_lo, w_hi, sigma);
        } else if (a.start_depth) {
            const double d = a.start_f32 ? (double)static_cast<const float *>(a.start_depth)[g] : static_cast<const double *>(a.start_depth)[g];
            if (d > 0.0 && d < __builtin_inf()) {
                const double w = 1.0 / d;
                p = PmPlane{w < w_lo ? w_lo : w > w_hi ? w_hi : w, 0.0, 0.0};
                have = true;
            }
        }
        if (!have) p = pm_draw(pm_key(a.seed, i, pix, 0), 0, w_lo, w_hi, sigma);
        const int n0 = a.nbr_start[i], len = a.nbr_start[i + 1] - n0;
        cost = pm_cost(a, n0, len, x, y, len > 0 ? pm_reference_bits(a, i, x, y) : 0, p);
    }
    a.plane[3 * g] = p.w, a.plane[3 * g + 1] = p.a, a.plane[3 * g + 2] = p.b;
    a.cost[g] = cost;
}

// One colour of iteration a.it: t = 1 + 2 it + colour.
__global__ __launch_bounds__(PM_THREADS) void pm_half_kernel(const PmArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.z, tid = threadIdx.x;
    const int half_log2 = a.tw_log2 - 1;                        // TW / 2 active pixels per row of the tile
    const int TW = 1 << a.tw_log2, TH = PM_TILE_PIXELS >> a.tw_log2;
    const int y = blockIdx.y * TH + (tid >> half_log2);
    const int x = blockIdx.x * TW + 2 * (tid & ((1 << half_log2) - 1)) + ((a.colour + y) & 1);   // the tile starts on an even column
    if (x >= a.W || y >= a.H || !pm_strict(a, x, y)) return;
    const int64_t HW = (int64_t)a.H * a.W, pix = (int64_t)y * a.W + x, g = (int64_t)i * HW + pix;
    const double *__restrict__ vw = a.view + (int64_t)i * PM_VIEW_WORDS;
    const double w_lo = vw[0], w_hi = vw[1], sigma = vw[2];
    const int n0 = a.nbr_start[i], len = a.nbr_start[i + 1] - n0;
    if (len == 0) return;   // every cost is 0: no candidate is strictly better
    const uint64_t ref = pm_reference_bits(a, i, x, y);
    const uint64_t key = pm_key(a.seed, i, pix, 1 + 2 * a.it + a.colour);
    const double rho = a.rho, half_it = a.half_it;
    PmPlane cur{a.plane[3 * g], a.plane[3 * g + 1], a.plane[3 * g + 2]};
    int cost = a.cost[g];
    for (int c = 0; c < 12; ++c) {   // one copy of the cost's code: the candidate is chosen by arithmetic on c
        PmPlane cand = cur;
        bool have = true;
        if (c < 8) {   // the plane of the pixel at (ox, oy), read here
            const int d = c < 4 ? 1 : 5, sgn = (c & 1) ? 1 : -1;
            const int ox = (c & 2) ? 0 : sgn * d, oy = (c & 2) ? sgn * d : 0;
            have = pm_strict(a, x + ox, y + oy);
            if (have) {
                const double *__restrict__ q = a.plane + 3 * (g + (int64_t)oy * a.W + ox);
                cand = PmPlane{(q[0] - q[1] * (double)ox) - q[2] * (double)oy, q[1], q[2]};
            }
        } else if (c == 11) {
            cand = pm_draw(key, 6, w_lo, w_hi, sigma);
        } else {
            const double delta = (sigma * cur.w) * half_it;
            if (c == 8) cand.w = cur.w * (1.0 + rho * (2.0 * pm_rand(key, 0) - 1.0));
            if (c == 9) cand.a = cur.a + delta * (2.0 * pm_rand(key, 1) - 1.0), cand.b = cur.b + delta * (2.0 * pm_rand(key, 2) - 1.0);
            if (c == 10) {
                cand.w = cur.w * (1.0 + rho * (2.0 * pm_rand(key, 3) - 1.0));
                cand.a = cur.a + delta * (2.0 * pm_rand(key, 4) - 1.0), cand.b = cur.b + delta * (2.0 * pm_rand(key, 5) - 1.0);
            }
        }
        if (!have || !pm_admissible(cand, w_lo, w_hi, sigma)) continue;
        const int C = pm_cost(a, n0, len, x, y, ref, cand);
        if (C < cost) cur = cand, cost = C;
    }
    a.plane[3 * g] = cur.w, a.plane[3 * g + 1] = cur.a, a.plane[3 * g + 2] = cur.b;
    a.cost[g] = cost;
}

__global__ __launch_bounds__(PM_THREADS) void pm_finish_kernel(const PmArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.z, x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const int64_t g = (int64_t)i * a.H * a.W + (int64_t)y * a.W + x;
    const int len = a.nbr_start[i + 1] - a.nbr_start[i];
    const int status = !pm_strict(a, x, y) ? PM_NOT_STRICT : a.cost[g] >= a.tau * len ? PM_NO_VIEW : 0;
    const double nan = __builtin_nan("");
    double depth = nan, nx = nan, ny = nan, nz = nan;
    if (status == 0) {
        const double *__restrict__ vw = a.view + (int64_t)i * PM_VIEW_WORDS;
        const double w = a.plane[3 * g], pa = a.plane[3 * g + 1], pb = a.plane[3 * g + 2];
        depth = 1.0 / w;
        const double m0 = pa * vw[3], m1 = pb * vw[5], m2 = (w + pa * (vw[4] - (double)x)) + pb * (vw[6] - (double)y);
        const double len2 = (m0 * m0 + m1 * m1) + m2 * m2, l = sqrt(len2);
        nx = -m0 / l, ny = -m1 / l, nz = -m2 / l;
    }
    if (a.out_f32) static_cast<float *>(a.depth)[g] = (float)depth;
    else static_cast<double *>(a.depth)[g] = depth;
    if (a.normal) {
        if (a.out_f32) {
            float *n = static_cast<float *>(a.normal) + 3 * g;
            n[0] = (float)nx, n[1] = (float)ny, n[2] = (float)nz;
        } else {
            double *n = static_cast<double *>(a.normal) + 3 * g;
            n[0] = nx, n[1] = ny, n[2] = nz;
        }
    }
    if (a.status) a.status[g] = (uint8_t)status;
}

}  // namespace pcs
