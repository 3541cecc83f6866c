// ba_fusion.hpp — depth-map fusion across views: the geometric consistency check and the merged point (include/pcs_hip.h, "Depth-map
// fusion"; host side: pcs_fusion.inc).  Two launches.  fuse_check_kernel: one thread per reference pixel, a workgroup
// a FUSE_TX x FUSE_TY tile of ONE view, so that the view and its neighbour list are the same in every lane — the view tables are read
// at wave-uniform addresses, once per (workgroup, neighbour) — and the gathers of a tile fall into a compact patch of each neighbour's
// map.  fuse_unique_kernel: the opt-in duplicate marking, which needs the first launch's decision of EVERY view; the hand-over is the
// 4-byte support word per pixel.
//
// Every function below switches floating-point contraction OFF: the rule is a sequence of plain IEEE-754 double operations in the order
// written, so the partner pixel q the second launch recomputes has the bits the first launch saw, whatever either kernel does around
// the shared functions.  No atomics, every sum in list order: two runs give identical bits.  The neighbour list is walked with a loop
// over the CSR range; nothing per lane is indexed at run time ("Dense stereo": such arrays went to scratch).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcs {

constexpr int FUSE_TX = 32, FUSE_TY = 8;   // the tile: a wave is two rows of 32 pixels
constexpr int FUSE_MAX_NBR = 32;           // the width of the support word
enum : int { FUSE_INVALID = 1, FUSE_FEW = 2, FUSE_DUPLICATE = 4 };

struct FuseView {
    double fx, cx, fy, cy, r[9], t[3];   // K = [fx, cx, fy, cy]; [R | t] world -> view, R row-major
};

struct FuseArgs {
    const double *views;        // (V, 16): fx, cx, fy, cy, then the 3 x 4 [R | t] row-major
    const int32_t *nbr_start;   // (V + 1)
    const int32_t *nbr;
    const void *depth;          // (V, H, W) float or double
    int W, H, min_views;
    double px_tol2, rel_tol;
    const double *T;            // 12 doubles on the device or NULL
    void *pts;                  // (V, H, W, 3)
    int f32;
    uint8_t *mask;              // (V, H, W)
    uint8_t *count, *status;    // (V, H, W) or NULL
    uint32_t *support;          // (V, H, W): the caller's or the handle's, never NULL
    void *fused;                // (V, H, W) or NULL
    int fused_f32;
};

// the table row of view v: a wave-uniform address
__device__ __forceinline__ FuseView fuse_load_view(const double *__restrict__ views, int v) {
    const double *__restrict__ p = views + 16 * (int64_t)v;
    FuseView o;
    o.fx = p[0], o.cx = p[1], o.fy = p[2], o.cy = p[3];
    for (int k = 0; k < 9; ++k) o.r[k] = p[4 + k + k / 3];
    o.t[0] = p[7], o.t[1] = p[11], o.t[2] = p[15];
    return o;
}

// invalid: NaN, +-inf or <= 0
__device__ __forceinline__ bool fuse_depth_valid(double z) { return z > 0.0 && z < __builtin_inf(); }

// pixel (x, y) at z-depth z of view v -> the world: X = R^T (z ((x - cx) / fx, (y - cy) / fy, 1) - t)
__device__ __forceinline__ void fuse_to_world(const FuseView &v, double x, double y, double z, double &X0, double &X1, double &X2) {
#pragma clang fp contract(off)
    const double c0 = z * ((x - v.cx) / v.fx) - v.t[0];
    const double c1 = z * ((y - v.cy) / v.fy) - v.t[1];
    const double c2 = z - v.t[2];
    X0 = (v.r[0] * c0 + v.r[3] * c1) + v.r[6] * c2;
    X1 = (v.r[1] * c0 + v.r[4] * c1) + v.r[7] * c2;
    X2 = (v.r[2] * c0 + v.r[5] * c1) + v.r[8] * c2;
}

// the world -> view v: Y = R X + t
__device__ __forceinline__ void fuse_to_view(const FuseView &v, double X0, double X1, double X2, double &Y0, double &Y1, double &Y2) {
#pragma clang fp contract(off)
    Y0 = ((v.r[0] * X0 + v.r[1] * X1) + v.r[2] * X2) + v.t[0];
    Y1 = ((v.r[3] * X0 + v.r[4] * X1) + v.r[5] * X2) + v.t[1];
    Y2 = ((v.r[6] * X0 + v.r[7] * X1) + v.r[8] * X2) + v.t[2];
}

// the projection of Y by K of view v (the caller has checked Y2 > 0)
__device__ __forceinline__ void fuse_project(const FuseView &v, double Y0, double Y1, double Y2, double &u, double &w) {
#pragma clang fp contract(off)
    u = v.fx * (Y0 / Y2) + v.cx;
    w = v.fy * (Y1 / Y2) + v.cy;
}

// the partner pixel of world point X in view v: q = (floor(u + 0.5), floor(w + 0.5)); false behind the view or outside the image.  The
// comparisons are written so that a NaN fails, and q is converted only once it is known to lie inside.
__device__ __forceinline__ bool fuse_partner(const FuseView &v, double X0, double X1, double X2, int W, int H, int &qx, int &qy) {
#pragma clang fp contract(off)
    double Y0, Y1, Y2, u, w;
    fuse_to_view(v, X0, X1, X2, Y0, Y1, Y2);
    if (!(Y2 > 0.0)) return false;
    fuse_project(v, Y0, Y1, Y2, u, w);
    const double fu = floor(u + 0.5), fw = floor(w + 0.5);
    if (!(fu >= 0.0 && fu < (double)W && fw >= 0.0 && fw < (double)H)) return false;
    qx = (int)fu, qy = (int)fw;
    return true;
}

template <class T>
__global__ __launch_bounds__(FUSE_TX *FUSE_TY) void fuse_check_kernel(const FuseArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.z;
    const int x = blockIdx.x * FUSE_TX + threadIdx.x, y = blockIdx.y * FUSE_TY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const int64_t HW = (int64_t)a.H * a.W, g = (int64_t)i * HW + (int64_t)y * a.W + x;
    const T *__restrict__ D = static_cast<const T *>(a.depth);
    const double z = (double)D[g], xd = (double)x, yd = (double)y;
    const bool valid = fuse_depth_valid(z);
    const FuseView vi = fuse_load_view(a.views, i);
    const int k0 = a.nbr_start[i], k1 = a.nbr_start[i + 1];
    double X0, X1, X2;
    fuse_to_world(vi, xd, yd, z, X0, X1, X2);
    double S0 = X0, S1 = X1, S2 = X2;
    uint32_t support = 0;
    for (int k = k0; k < k1; ++k) {   // the same trip count and the same neighbour in every lane
        const int j = a.nbr[k];
        const FuseView vj = fuse_load_view(a.views, j);
        int qx = 0, qy = 0;
        bool ok = valid && fuse_partner(vj, X0, X1, X2, a.W, a.H, qx, qy);
        double zj = 0.0;
        if (ok) zj = (double)D[(int64_t)j * HW + (int64_t)qy * a.W + qx];
        ok = ok && fuse_depth_valid(zj);
        double P0, P1, P2, B0, B1, B2, xr, yr;
        fuse_to_world(vj, (double)qx, (double)qy, zj, P0, P1, P2);
        fuse_to_view(vi, P0, P1, P2, B0, B1, B2);
        ok = ok && B2 > 0.0;
        fuse_project(vi, B0, B1, B2, xr, yr);
        const double dx = xr - xd, dy = yr - yd;
        ok = ok && dx * dx + dy * dy <= a.px_tol2 && fabs(B2 - z) <= a.rel_tol * z;
        if (ok) {
            support |= 1u << (k - k0);
            S0 = S0 + P0, S1 = S1 + P1, S2 = S2 + P2;
        }
    }
    const int count = __popc(support);
    const bool kept = valid && count >= a.min_views;
    const double nan = __builtin_nan("");
    const double m = (double)(count + 1);
    const double F0 = S0 / m, F1 = S1 / m, F2 = S2 / m;
    double o0 = nan, o1 = nan, o2 = nan, fz = nan;
    if (kept) {
        o0 = F0, o1 = F1, o2 = F2;
        if (a.T) {
            const double *__restrict__ Tm = a.T;
            o0 = ((Tm[0] * F0 + Tm[1] * F1) + Tm[2] * F2) + Tm[3];
            o1 = ((Tm[4] * F0 + Tm[5] * F1) + Tm[6] * F2) + Tm[7];
            o2 = ((Tm[8] * F0 + Tm[9] * F1) + Tm[10] * F2) + Tm[11];
        }
        fz = ((vi.r[6] * F0 + vi.r[7] * F1) + vi.r[8] * F2) + vi.t[2];
    }
    a.support[g] = support;
    if (a.f32) {
        float *o = static_cast<float *>(a.pts) + 3 * g;
        o[0] = (float)o0, o[1] = (float)o1, o[2] = (float)o2;
    } else {
        double *o = static_cast<double *>(a.pts) + 3 * g;
        o[0] = o0, o[1] = o1, o[2] = o2;
    }
    a.mask[g] = (uint8_t)kept;
    if (a.count) a.count[g] = (uint8_t)count;
    if (a.status) a.status[g] = (uint8_t)(!valid ? FUSE_INVALID : kept ? 0 : FUSE_FEW);
    if (a.fused) {
        if (a.fused_f32) static_cast<float *>(a.fused)[g] = (float)fz;
        else static_cast<double *>(a.fused)[g] = fz;
    }
}

// Behind fuse_check_kernel of every view.  A kept pixel becomes a duplicate when the partner pixel q of a consistent neighbour j < i is
// itself kept by the first launch: its support word has at least min_views bits (an invalid pixel's word is 0).  Only the support
// words are read and only this pixel's outputs are written, so the result does not depend on an order of evaluation.
template <class T>
__global__ __launch_bounds__(FUSE_TX *FUSE_TY) void fuse_unique_kernel(const FuseArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.z;
    const int x = blockIdx.x * FUSE_TX + threadIdx.x, y = blockIdx.y * FUSE_TY + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const int64_t HW = (int64_t)a.H * a.W, g = (int64_t)i * HW + (int64_t)y * a.W + x;
    const uint32_t *__restrict__ sup = a.support;
    const uint32_t support = sup[g];
    const bool kept = __popc(support) >= a.min_views;
    const T *__restrict__ D = static_cast<const T *>(a.depth);
    const double z = kept ? (double)D[g] : 1.0;
    const FuseView vi = fuse_load_view(a.views, i);
    const int k0 = a.nbr_start[i], k1 = a.nbr_start[i + 1];
    double X0, X1, X2;
    fuse_to_world(vi, (double)x, (double)y, z, X0, X1, X2);
    bool dup = false;
    for (int k = k0; k < k1; ++k) {
        const int j = a.nbr[k];
        if (j >= i) continue;   // the same in every lane
        const FuseView vj = fuse_load_view(a.views, j);
        int qx = 0, qy = 0;
        const bool ok = kept && ((support >> (k - k0)) & 1u) && fuse_partner(vj, X0, X1, X2, a.W, a.H, qx, qy);
        if (ok && __popc(sup[(int64_t)j * HW + (int64_t)qy * a.W + qx]) >= a.min_views) dup = true;
    }
    if (!dup) return;
    if (a.f32) {
        float *o = static_cast<float *>(a.pts) + 3 * g;
        o[0] = o[1] = o[2] = __builtin_nanf("");
    } else {
        double *o = static_cast<double *>(a.pts) + 3 * g;
        o[0] = o[1] = o[2] = __builtin_nan("");
    }
    a.mask[g] = 0;
    if (a.status) a.status[g] = (uint8_t)FUSE_DUPLICATE;
    if (a.fused) {
        if (a.fused_f32) static_cast<float *>(a.fused)[g] = __builtin_nanf("");
        else static_cast<double *>(a.fused)[g] = __builtin_nan("");
    }
}

}  // namespace pcs
