// ba_tsdf_colour.hpp — the images brought back onto the surface: a colour per point from the source views that see it
// (include/pcs_hip.h, "Colour of surface points from the images"; host side: pcs_tsdf.inc).
//
// tsdf_colour_view_sample is THE per-(point, view) function: transform and projection of ba_fusion.hpp (fuse_to_view, fuse_project),
// the in-image test, the visibility test against the view's depth map at the nearest pixel, the angle test against the normal, and
// the bilinear sample.  Both colour kernels run it through tsdf_colour_point, which holds the loop over the views INSIDE the thread,
// in list order, with the running sums in registers: the combination is deterministic and needs no atomics.  The view row of the
// current iteration is the same in every lane (a wave-uniform address, as in tsdf_integrate_kernel); the loop bound is the
// host-checked n_views.
//   tsdf_colour_points_kernel   one thread per caller-supplied point
//   tsdf_colour_views_kernel    one thread per pixel of a render view; a workgroup is a 16 x 16 tile of ONE view and each wave an 8 x 8
//                               quadrant, as in tsdf_raycast_kernel.  The point is C + z w by the cast's ray formulas.
//   tsdf_point_normals_kernel   the cast's normal rule at arbitrary points, through the cast's own T(g) (tsdf_ray_normal)
// Channels unroll by template over {1, 3, 4}: nothing per lane is indexed at run time (no scratch).  Every index is int64_t.  Pixel
// indices are clamped in double before they are converted, so no coordinate, a NaN included, forms an address outside an image or a
// map; the loads themselves run only for a (point, view) that passed every test.
//
// Contraction is off in every function: plain IEEE-754 double operations in the order written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_fusion.hpp"
#include "ba_tsdf_raycast.hpp"

namespace pcs {

constexpr int TSDF_COLOUR_ROW = 20;      // doubles per source view: the 16 of pcs_fuse_set_views, the centre C, one unused
constexpr int TSDF_COLOUR_BLOCK = 256;   // points per workgroup
enum : int { TSDF_COLOUR_BLEND = 0, TSDF_COLOUR_BEST = 1 };

struct TsdfColourArgs {
    const double *views;     // (V, TSDF_COLOUR_ROW)
    int n_views, W, H;       // the source views' common size, both sides >= 2
    const void *images;      // (V, H, pitch BYTES)
    int64_t pitch;
    const void *vis;         // (V, H, W) float or double; read by the VIS instantiations only
    int vis_f32;
    double tol, cos_min;
    int mode;
    double fill[4];
    int64_t n;               // points
    const void *points;      // (n, 3); the points kernel
    const float *normals;    // (n, 3), or (R, RH, RW, 3) for the views kernel; read by the NRM instantiations only
    const double *rviews;    // (R, 16): the render rows of the cast; the views kernel
    const void *depth;       // (R, RH, RW)
    int RW, RH;
    void *colour;            // (n, C) or (R, RH, RW, C), uint8 or float
    int colour_f32;
    float *weight;           // or NULL
    uint16_t *count;         // or NULL
    int32_t *best;           // or NULL
};

struct TsdfPointNormalArgs {
    TsdfRaycastArgs field;   // sum, weight, g and min_weight: what T(g) reads
    int64_t n;
    const void *points;      // (n, 3)
    float *normals;          // (n, 3)
    uint8_t *status;         // (n) or NULL
};

// min(max(c, 0), top) decided in double (a NaN gives 0) and converted once it lies inside
__device__ __forceinline__ int tsdf_colour_clamp(double c, int top) {
    c = c > 0.0 ? c : 0.0;
    const double t = (double)top;
    c = c < t ? c : t;
    return (int)c;
}

__device__ __forceinline__ double tsdf_colour_value(const uint8_t *p, int k) { return (double)p[k]; }
__device__ __forceinline__ double tsdf_colour_value(const float *p, int k) { return (double)p[k]; }

// One point against one view: false when the view does not contribute; else c, the weight, and I, the sample per channel.
template <class TI, int C, bool VIS, bool NRM>
__device__ __forceinline__ bool tsdf_colour_view_sample(const TsdfColourArgs &a, int v, double X0, double X1, double X2, double n0, double n1, double n2, double &c,
                                                        double (&I)[C]) {
#pragma clang fp contract(off)
    const double *__restrict__ row = a.views + TSDF_COLOUR_ROW * (int64_t)v;   // the same address in every lane
    const FuseView vw = fuse_load_view(row, 0);
    double Y0, Y1, Y2, u, w;
    fuse_to_view(vw, X0, X1, X2, Y0, Y1, Y2);
    bool ok = Y2 > 0.0;
    fuse_project(vw, Y0, Y1, Y2, u, w);
    ok = ok && u >= 0.0 && u <= (double)(a.W - 1) && w >= 0.0 && w <= (double)(a.H - 1);
    if (VIS) {
        const int qx = tsdf_colour_clamp(floor(u + 0.5), a.W - 1), qy = tsdf_colour_clamp(floor(w + 0.5), a.H - 1);
        const int64_t q = ((int64_t)v * a.H + qy) * a.W + qx;
        double d = 0.0;
        if (ok) d = a.vis_f32 ? (double)static_cast<const float *>(a.vis)[q] : static_cast<const double *>(a.vis)[q];
        ok = ok && fuse_depth_valid(d) && Y2 <= d + a.tol;
    }
    c = 1.0;
    if (NRM) {
        const double e0 = row[16] - X0, e1 = row[17] - X1, e2 = row[18] - X2;
        const double len = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        c = ((n0 * e0 + n1 * e1) + n2 * e2) / len;
        ok = ok && c > a.cos_min;   // a NaN fails
    }
    const int x0 = tsdf_colour_clamp(floor(u), a.W - 2), y0 = tsdf_colour_clamp(floor(w), a.H - 2);
    const double fx = u - (double)x0, fy = w - (double)y0, ex = 1.0 - fx, ey = 1.0 - fy;
    const uint8_t *base = static_cast<const uint8_t *>(a.images) + ((int64_t)v * a.H + y0) * a.pitch + (int64_t)x0 * (int64_t)(C * sizeof(TI));
    const TI *__restrict__ r0 = reinterpret_cast<const TI *>(base), *__restrict__ r1 = reinterpret_cast<const TI *>(base + a.pitch);
#pragma unroll
    for (int k = 0; k < C; ++k) {
        double s = 0.0;
        if (ok) {
            const double top = tsdf_lerp(ex, fx, tsdf_colour_value(r0, k), tsdf_colour_value(r0, C + k));
            const double bot = tsdf_lerp(ex, fx, tsdf_colour_value(r1, k), tsdf_colour_value(r1, C + k));
            s = tsdf_lerp(ey, fy, top, bot);
        }
        I[k] = s;
    }
    return ok;
}

__device__ __forceinline__ void tsdf_colour_store(void *colour, int f32, int64_t i, double v) {
    if (f32) static_cast<float *>(colour)[i] = (float)v;
    else static_cast<uint8_t *>(colour)[i] = (uint8_t)fmin(fmax(rint(v), 0.0), 255.0);   // half-to-even, saturated; NaN -> 0
}

// The loop over the views for one point and its outputs at position p.  `live` false: no view is asked (the fill).
template <class TI, int C, bool VIS, bool NRM>
__device__ __forceinline__ void tsdf_colour_point(const TsdfColourArgs &a, int64_t p, bool live, double X0, double X1, double X2, double n0, double n1, double n2) {
#pragma clang fp contract(off)
    double S[C];
#pragma unroll
    for (int k = 0; k < C; ++k) S[k] = 0.0;
    double Wt = 0.0, best_c = 0.0;
    int best = -1;
    unsigned count = 0;
    const bool pick = a.mode == TSDF_COLOUR_BEST;
    for (int v = 0; v < a.n_views; ++v) {   // the same trip count and the same view in every lane
        double c, I[C];
        const bool ok = tsdf_colour_view_sample<TI, C, VIS, NRM>(a, v, X0, X1, X2, n0, n1, n2, c, I) && live;
        if (ok) {
            const bool better = best < 0 || c > best_c;   // a tie stays with the lower list position
            if (better) best = v, best_c = c;
#pragma unroll
            for (int k = 0; k < C; ++k) {
                if (pick) S[k] = better ? I[k] : S[k];
                else S[k] = S[k] + c * I[k];
            }
            Wt = Wt + c;
            count += 1u;
        }
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
        const double val = count == 0 ? a.fill[k] : pick ? S[k] : S[k] / Wt;
        tsdf_colour_store(a.colour, a.colour_f32, p * C + k, val);
    }
    if (a.weight) a.weight[p] = (float)Wt;
    if (a.count) a.count[p] = (uint16_t)count;
    if (a.best) a.best[p] = best;
}

template <class TI, class TP, int C, bool VIS, bool NRM>
__global__ __launch_bounds__(TSDF_COLOUR_BLOCK) void tsdf_colour_points_kernel(const TsdfColourArgs a) {
    const int64_t p = (int64_t)blockIdx.x * TSDF_COLOUR_BLOCK + threadIdx.x;
    if (p >= a.n) return;
    const TP *__restrict__ X = static_cast<const TP *>(a.points) + 3 * p;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (NRM) n0 = (double)a.normals[3 * p], n1 = (double)a.normals[3 * p + 1], n2 = (double)a.normals[3 * p + 2];
    tsdf_colour_point<TI, C, VIS, NRM>(a, p, true, (double)X[0], (double)X[1], (double)X[2], n0, n1, n2);
}

template <class TI, class TD, int C, bool VIS, bool NRM>
__global__ __launch_bounds__(TSDF_RAY_BLOCK *TSDF_RAY_BLOCK) void tsdf_colour_views_kernel(const TsdfColourArgs a) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int x = blockIdx.x * TSDF_RAY_BLOCK + (wave & 1) * TSDF_RAY_TILE + (lane & (TSDF_RAY_TILE - 1));
    const int y = blockIdx.y * TSDF_RAY_BLOCK + (wave >> 1) * TSDF_RAY_TILE + (lane >> 3);
    if (x >= a.RW || y >= a.RH) return;
    const int r = blockIdx.z;
    const double *__restrict__ row = a.rviews + 16 * (int64_t)r;   // the same address in every lane
    const double fx = row[0], cx = row[1], fy = row[2], cy = row[3];
    const double r0 = ((double)x - cx) / fx, r1 = ((double)y - cy) / fy;
    const double w0 = (row[4] * r0 + row[7] * r1) + row[10] * 1.0;
    const double w1 = (row[5] * r0 + row[8] * r1) + row[11] * 1.0;
    const double w2 = (row[6] * r0 + row[9] * r1) + row[12] * 1.0;
    const int64_t p = ((int64_t)r * a.RH + y) * a.RW + x;
    const double z = (double)static_cast<const TD *>(a.depth)[p];
    const bool live = fuse_depth_valid(z);
    const double X0 = row[13] + z * w0, X1 = row[14] + z * w1, X2 = row[15] + z * w2;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (NRM) n0 = (double)a.normals[3 * p], n1 = (double)a.normals[3 * p + 1], n2 = (double)a.normals[3 * p + 2];
    tsdf_colour_point<TI, C, VIS, NRM>(a, p, live, X0, X1, X2, n0, n1, n2);
}

template <class S, class TP>
__global__ __launch_bounds__(TSDF_COLOUR_BLOCK) void tsdf_point_normals_kernel(const TsdfPointNormalArgs a) {
#pragma clang fp contract(off)
    const int64_t p = (int64_t)blockIdx.x * TSDF_COLOUR_BLOCK + threadIdx.x;
    if (p >= a.n) return;
    const TP *__restrict__ X = static_cast<const TP *>(a.points) + 3 * p;
    const TsdfGrid &g = a.field.g;
    const double g0 = ((double)X[0] - g.o[0]) / g.s, g1 = ((double)X[1] - g.o[1]) / g.s, g2 = ((double)X[2] - g.o[2]) / g.s;
    const double nan = __builtin_nan("");
    double n0 = nan, n1 = nan, n2 = nan;
    unsigned evaluated = 0;
    bool ok = g.nx >= 2 && g.ny >= 2 && g.nz >= 2;   // no cells: no sample can be taken
    ok = ok && tsdf_ray_normal<S>(a.field, g0, g1, g2, n0, n1, n2, evaluated);
    float *o = a.normals + 3 * p;
    o[0] = (float)n0, o[1] = (float)n1, o[2] = (float)n2;
    if (a.status) a.status[p] = ok ? 0 : 1;
}

}  // namespace pcs
