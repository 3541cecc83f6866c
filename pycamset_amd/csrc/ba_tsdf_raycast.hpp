// ba_tsdf_raycast.hpp — the TSDF volume rendered back into a camera: depth and normal maps of any view by marching the distance field
// (include/pcs_hip.h, "Ray-cast of the TSDF volume"; host side: pcs_tsdf.inc).
//
// tsdf_raycast_kernel: one thread per pixel.  A workgroup is a 16 x 16 pixel tile of ONE view and each of its four waves an 8 x 8
// quadrant of it, not a 64 x 1 strip: the 64 rays of a wave stay a compact bundle as they advance, so their eight-corner gathers fall
// into few cache lines of the volume.  The view's 16 doubles are read at a wave-uniform address (blockIdx.z), as in
// tsdf_integrate_kernel.  The march is an integer loop over n = 0 .. N with N fixed before the loop; every sample position is z0 + n dz,
// a product, so a sample does not depend on which samples before it were evaluated.  Nothing per lane is indexed at run time (no
// scratch), there are no atomics, and every node index is int64_t.
//
// tsdf_brick_mask_kernel: one thread per node, x fastest.  A brick is 8^3 cells; its flag says that one of its corner nodes is observed
// with sum <= 0.  A node is a corner of the cells one below and at its own index on each axis, so it marks up to eight bricks.  Every
// writer stores the same byte 1 into a mask the host zeroed: plain stores, whichever lands first.  The mask depends on min_weight, so
// it is made once per call.
//
// Skipping changes no bit.  With f in [0, 1] the blend (1 - f) A + f B of two numbers > 0 is > 0, so a VALID sample whose cell lies in
// an unflagged brick is > 0: it can never be the second sample of a hit and is not evaluated.  It can be the first: on reaching a
// sample in a flagged brick whose predecessor was skipped, the predecessor is evaluated for real.
//
// The instantiation with COUNT set is the bench's separate counting launch: the same march, which writes per pixel the number of
// samples it evaluated (march and normal) and none of the three outputs.  The shipped path counts nothing.
//
// Contraction is off in every function: plain IEEE-754 double operations in the order written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_tsdf.hpp"

namespace pcs {

constexpr int TSDF_RAY_TILE = 8;          // a wave: TILE x TILE pixels
constexpr int TSDF_RAY_BLOCK = 16;        // a workgroup: BLOCK x BLOCK pixels, four waves
constexpr int TSDF_BRICK_SHIFT = 3;       // a brick: 8^3 cells
constexpr int TSDF_RAY_MAX_STEPS = 113513;   // 64 sqrt(3) 1024 + 1, rounded up: the largest N the limits admit
enum : int { TSDF_RAY_HIT = 0, TSDF_RAY_NO_NORMAL = 1, TSDF_RAY_NO_CROSSING = 2, TSDF_RAY_MISSED = 3 };

struct TsdfRaycastArgs {
    const double *views;     // (V, 16): fx, cx, fy, cy, the nine entries of R row-major, the centre C
    const void *sum;
    const uint16_t *weight;
    const uint8_t *mask;     // (bz, by, bx) brick flags, or NULL: every sample is evaluated
    TsdfGrid g;
    int bx, by;
    int W, H, min_weight;
    double step, z_near, z_far;
    void *depth;             // (V, H, W) float or double
    float *normal;           // (V, H, W, 3) or NULL
    uint8_t *status;         // (V, H, W) or NULL
    uint32_t *samples;       // (V, H, W): the counting launch only
};

struct TsdfMaskArgs {
    const void *sum;
    const uint16_t *weight;
    TsdfGrid g;
    int bx, by, bz, min_weight;
    uint8_t *mask;
};

// the two bricks (equal at most places) that hold the cells node index i is a corner of: cells i - 1 and i, where they exist
__device__ __forceinline__ void tsdf_node_bricks(int i, int n, int &b0, int &b1) {
    const int c0 = i > 0 ? i - 1 : 0, c1 = i < n - 2 ? i : n - 2;
    b0 = c0 >> TSDF_BRICK_SHIFT, b1 = c1 >> TSDF_BRICK_SHIFT;
}

template <class S>
__global__ __launch_bounds__(TSDF_TX *TSDF_TY) void tsdf_brick_mask_kernel(const TsdfMaskArgs a) {
    const int i = blockIdx.x * TSDF_TX + threadIdx.x, j = blockIdx.y * TSDF_TY + threadIdx.y, k = blockIdx.z;
    if (i >= a.g.nx || j >= a.g.ny) return;
    const int64_t n = ((int64_t)k * a.g.ny + j) * a.g.nx + i;
    if (a.weight[n] < (unsigned)a.min_weight) return;
    if (!((double)static_cast<const S *>(a.sum)[n] <= 0.0)) return;
    int i0, i1, j0, j1, k0, k1;   // n_a >= 2 on every axis: the host launches nothing otherwise
    tsdf_node_bricks(i, a.g.nx, i0, i1), tsdf_node_bricks(j, a.g.ny, j0, j1), tsdf_node_bricks(k, a.g.nz, k0, k1);
    for (int kk = k0; kk <= k1; ++kk)
        for (int jj = j0; jj <= j1; ++jj)
            for (int ii = i0; ii <= i1; ++ii) a.mask[((int64_t)kk * a.by + jj) * a.bx + ii] = 1;
}

// the cell index along one axis: min(max(floor(g), 0), n - 2), decided in double (a NaN gives 0) and converted once it lies inside
__device__ __forceinline__ int tsdf_ray_cell(double g, int n) {
    double c = floor(g);
    c = c > 0.0 ? c : 0.0;
    const double top = (double)(n - 2);
    c = c < top ? c : top;
    return (int)c;
}

__device__ __forceinline__ double tsdf_ray_frac(double g, int c) {
#pragma clang fp contract(off)
    double f = g - (double)c;
    f = f > 0.0 ? f : 0.0;
    return f < 1.0 ? f : 1.0;
}

__device__ __forceinline__ double tsdf_lerp(double f1, double f, double A, double B) {
#pragma clang fp contract(off)
    return f1 * A + f * B;
}

// T(g): VALID iff the eight corners of the cell are observed; the value is the trilinear blend along x, then y, then z
template <class S>
__device__ __forceinline__ bool tsdf_ray_sample(const TsdfRaycastArgs &a, int c0, int c1, int c2, double g0, double g1, double g2, double &T) {
#pragma clang fp contract(off)
    const S *__restrict__ sum = static_cast<const S *>(a.sum);
    const int64_t sy = a.g.nx, sz = (int64_t)a.g.nx * a.g.ny;
    const int64_t n = ((int64_t)c2 * a.g.ny + c1) * a.g.nx + c0;
    double D[8];
    bool all = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t m = n + (c & 1) + (c >> 1 & 1) * sy + (c >> 2 & 1) * sz;
        const unsigned w = a.weight[m];
        all = all && w >= (unsigned)a.min_weight;
        D[c] = (double)sum[m] / (double)w;
    }
    const double f0 = tsdf_ray_frac(g0, c0), f1 = tsdf_ray_frac(g1, c1), f2 = tsdf_ray_frac(g2, c2);
    const double e0 = 1.0 - f0, e1 = 1.0 - f1, e2 = 1.0 - f2;
    const double x0 = tsdf_lerp(e0, f0, D[0], D[1]), x1 = tsdf_lerp(e0, f0, D[2], D[3]), x2 = tsdf_lerp(e0, f0, D[4], D[5]), x3 = tsdf_lerp(e0, f0, D[6], D[7]);
    const double y0 = tsdf_lerp(e1, f1, x0, x1), y1 = tsdf_lerp(e1, f1, x2, x3);
    T = tsdf_lerp(e2, f2, y0, y1);
    return all;
}

template <class S>
__device__ __forceinline__ bool tsdf_ray_sample_at(const TsdfRaycastArgs &a, double g0, double g1, double g2, double &T) {
    return tsdf_ray_sample<S>(a, tsdf_ray_cell(g0, a.g.nx), tsdf_ray_cell(g1, a.g.ny), tsdf_ray_cell(g2, a.g.nz), g0, g1, g2, T);
}

// a sample of the normal: it must lie in the box on every axis (a NaN fails) and be VALID
template <class S>
__device__ __forceinline__ bool tsdf_ray_normal_sample(const TsdfRaycastArgs &a, double g0, double g1, double g2, double &T, unsigned &evaluated) {
    const double h0 = (double)(a.g.nx - 1), h1 = (double)(a.g.ny - 1), h2 = (double)(a.g.nz - 1);
    if (!(g0 >= 0.0 && g0 <= h0 && g1 >= 0.0 && g1 <= h1 && g2 >= 0.0 && g2 <= h2)) return false;
    evaluated += 1u;
    return tsdf_ray_sample_at<S>(a, g0, g1, g2, T);
}

// the normal at grid point g: central differences of T one node apart, taken in the order +x, -x, +y, -y, +z, -z; false (n untouched)
// when one of the six samples fails or |G| is not > 0.  Shared with tsdf_point_normals_kernel (ba_tsdf_colour.hpp).
template <class S>
__device__ __forceinline__ bool tsdf_ray_normal(const TsdfRaycastArgs &a, double g0, double g1, double g2, double &n0, double &n1, double &n2, unsigned &evaluated) {
#pragma clang fp contract(off)
    double Ta, Tb, G0 = 0.0, G1 = 0.0, G2 = 0.0;
    bool ok = tsdf_ray_normal_sample<S>(a, g0 + 1.0, g1, g2, Ta, evaluated) && tsdf_ray_normal_sample<S>(a, g0 - 1.0, g1, g2, Tb, evaluated);
    if (ok) G0 = Ta - Tb;
    ok = ok && tsdf_ray_normal_sample<S>(a, g0, g1 + 1.0, g2, Ta, evaluated) && tsdf_ray_normal_sample<S>(a, g0, g1 - 1.0, g2, Tb, evaluated);
    if (ok) G1 = Ta - Tb;
    ok = ok && tsdf_ray_normal_sample<S>(a, g0, g1, g2 + 1.0, Ta, evaluated) && tsdf_ray_normal_sample<S>(a, g0, g1, g2 - 1.0, Tb, evaluated);
    if (ok) G2 = Ta - Tb;
    const double len = sqrt((G0 * G0 + G1 * G1) + G2 * G2);
    ok = ok && len > 0.0;   // a NaN fails
    if (ok) n0 = G0 / len, n1 = G1 / len, n2 = G2 / len;
    return ok;
}

// one axis of the clip: false when the ray runs along the axis outside the slab
__device__ __forceinline__ bool tsdf_ray_clip(double gc, double gw, int n, double &z0, double &z1) {
#pragma clang fp contract(off)
    const double h = (double)(n - 1);
    if (gw == 0.0) return gc >= 0.0 && gc <= h;
    const double t0 = (0.0 - gc) / gw, t1 = (h - gc) / gw;
    const double lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
    z0 = lo > z0 ? lo : z0;
    z1 = hi < z1 ? hi : z1;
    return true;
}

template <class S, class TD, bool COUNT = false>
__global__ __launch_bounds__(TSDF_RAY_BLOCK *TSDF_RAY_BLOCK) void tsdf_raycast_kernel(const TsdfRaycastArgs a) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * TSDF_RAY_BLOCK + (wave & 1) * TSDF_RAY_TILE + (lane & (TSDF_RAY_TILE - 1));
    const int y = blockIdx.y * TSDF_RAY_BLOCK + (wave >> 1) * TSDF_RAY_TILE + (lane >> 3);
    if (x >= a.W || y >= a.H) return;
    const int v = blockIdx.z;
    const double *__restrict__ row = a.views + 16 * (int64_t)v;   // the same address in every lane
    const double fx = row[0], cx = row[1], fy = row[2], cy = row[3];
    const double r0 = ((double)x - cx) / fx, r1 = ((double)y - cy) / fy;
    // w_a = (R_0a r_0 + R_1a r_1) + R_2a r_2 with r_2 = 1
    const double w0 = (row[4] * r0 + row[7] * r1) + row[10] * 1.0;
    const double w1 = (row[5] * r0 + row[8] * r1) + row[11] * 1.0;
    const double w2 = (row[6] * r0 + row[9] * r1) + row[12] * 1.0;
    const double s = a.g.s;
    const double gc0 = (row[13] - a.g.o[0]) / s, gc1 = (row[14] - a.g.o[1]) / s, gc2 = (row[15] - a.g.o[2]) / s;
    const double gw0 = w0 / s, gw1 = w1 / s, gw2 = w2 / s;

    const double nan = __builtin_nan("");
    double depth = nan, n0 = nan, n1 = nan, n2 = nan;
    int status = TSDF_RAY_MISSED;
    unsigned evaluated = 0;   // read by the counting launch only
    double z0 = a.z_near, z1 = a.z_far;
    bool in = a.g.nx >= 2 && a.g.ny >= 2 && a.g.nz >= 2;
    in = in && tsdf_ray_clip(gc0, gw0, a.g.nx, z0, z1);
    in = in && tsdf_ray_clip(gc1, gw1, a.g.ny, z0, z1);
    in = in && tsdf_ray_clip(gc2, gw2, a.g.nz, z0, z1);
    in = in && z0 <= z1;
    const double dz = a.step / sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double q = (z1 - z0) / dz;
    in = in && q <= (double)TSDF_RAY_MAX_STEPS;   // a NaN fails: the loop below is bounded for any finite table
    if (in) {
        status = TSDF_RAY_NO_CROSSING;
        const int N = (int)floor(q);
        bool have_prev = false, prev_valid = false;   // have_prev: sample n - 1 was evaluated
        double prev_T = 0.0, prev_z = 0.0;
        for (int n = 0; n <= N; ++n) {
            const double z = z0 + (double)n * dz;
            const double g0 = gc0 + z * gw0, g1 = gc1 + z * gw1, g2 = gc2 + z * gw2;
            const int c0 = tsdf_ray_cell(g0, a.g.nx), c1 = tsdf_ray_cell(g1, a.g.ny), c2 = tsdf_ray_cell(g2, a.g.nz);
            if (a.mask) {
                const int64_t b = ((int64_t)(c2 >> TSDF_BRICK_SHIFT) * a.by + (c1 >> TSDF_BRICK_SHIFT)) * a.bx + (c0 >> TSDF_BRICK_SHIFT);
                if (!a.mask[b]) {
                    have_prev = false;
                    continue;
                }
                if (!have_prev && n >= 1) {   // the predecessor was skipped: it may be the first sample of a hit
                    prev_z = z0 + (double)(n - 1) * dz;
                    prev_valid = tsdf_ray_sample_at<S>(a, gc0 + prev_z * gw0, gc1 + prev_z * gw1, gc2 + prev_z * gw2, prev_T);
                    have_prev = true;
                    evaluated += 1u;
                }
            }
            double T;
            const bool valid = tsdf_ray_sample<S>(a, c0, c1, c2, g0, g1, g2, T);
            evaluated += 1u;
            if (have_prev && prev_valid && valid && prev_T > 0.0 && T <= 0.0) {
                depth = prev_z + dz * (prev_T / (prev_T - T));
                status = TSDF_RAY_HIT;
                break;
            }
            have_prev = true, prev_valid = valid, prev_T = T, prev_z = z;
        }
        if (status == TSDF_RAY_HIT && a.normal) {
            const double g0 = gc0 + depth * gw0, g1 = gc1 + depth * gw1, g2 = gc2 + depth * gw2;
            if (!tsdf_ray_normal<S>(a, g0, g1, g2, n0, n1, n2, evaluated)) status = TSDF_RAY_NO_NORMAL;
        }
    }
    const int64_t p = ((int64_t)v * a.H + y) * a.W + x;
    if (COUNT) {
        a.samples[p] = evaluated;
        return;
    }
    static_cast<TD *>(a.depth)[p] = (TD)depth;
    if (a.normal) {
        float *o = a.normal + 3 * p;
        o[0] = (float)n0, o[1] = (float)n1, o[2] = (float)n2;
    }
    if (a.status) a.status[p] = (uint8_t)status;
}

}  // namespace pcs
