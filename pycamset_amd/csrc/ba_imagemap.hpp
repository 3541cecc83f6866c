// ba_imagemap.hpp — a finished calibration applied to points and images.
//
// Reference: nb_undistort_arr / nb_distort (optimisation/compiled_helpers.py:373-490), sensor_map / vector_cam_points
// (utils/general_utils.py:432-483), Camera._compute_world_sensor_map / undistort / im_to_world_ray (cameras/camera.py:162-177,
// :451-493), undistort_im / remap_im / rectify_camera_images (reconstruction/reconstruction_utils.py:12-107), which lean on
// cv2.undistort, cv2.initUndistortRectifyMap and cv2.remap.
//
// Kernels (all coordinate arithmetic FP64; one camera table row of IMAP_CAM_STRIDE doubles per camera):
//   imap_points_kernel   one thread per point: undistort (five fixed-point steps by undistort5, another count by the same step run
//                        `iters` times), distort (the forward Brown-Conrady model of eval_detection), or the ray of a pixel.
//   imap_raymap_kernel   every pixel of a W x H sensor through the ray path, (H, W, 3) in image order; with a depth image the point
//                        position + ray * depth instead.
//   imap_build_maps_kernel  cv2.initUndistortRectifyMap: per destination pixel X = R_new^T K_new^-1 (u, v, 1), x = X / Z, y = Y / Z,
//                        forward distortion, the source camera's K; two planes (2, Hd, Wd).  Z <= 0 gives NaN.
//   imap_remap_kernel    cv2.remap, batched: n_img images of one shape, each with its own camera.  The source coordinate comes from
//                        the camera table in registers (fused: no map is ever written or read) or from a map.  One sampling routine.
//
// The remap's shape.  A lane owns IMAP_PX = 4 adjacent destination pixels of one row, so that 8-bit mono results leave as one dword
// (sub-dword stores waste the store path); the row tail and rows whose address is not dword-aligned take the element path.  A
// workgroup is 32 lanes x 8 rows = a 128 x 8 pixel tile: the source gather of a tile falls into a compact window of the source, and
// blockIdx.x runs along the row, so that workgroups dispatched together share source rows in L2.  The camera row is wave-uniform
// (one image per blockIdx.z) and is read through the scalar cache.
//
// Sampling rules (tests/imagemap_reference.py states them sequentially):
//   nearest   the tap at (rint(sx), rint(sy)), ties to even (cvRound);
//   bilinear  x0 = floor(sx), fx = sx - x0; rows first: r_j = t_j0 (1 - fx) + t_j1 fx, value = r_0 (1 - fy) + r_1 fy;
//   bicubic   x0 = floor(sx), taps x0 - 1 .. x0 + 2, Keys' kernel with a = -0.75 in the form cv2's interpolateCubic evaluates,
//             w_3 = 1 - w_0 - w_1 - w_2; rows first, taps in ascending order.
//   A tap outside the source takes the border value (BORDER_CONSTANT); valid = every tap inside.  Where NO tap is inside (a
//   coordinate far outside, or NaN) the value is the border value itself.  floor, not truncation, for negative coordinates.
//   uint8 results: the FP64 value rounded half-to-even and saturated; float results: rounded once at the store.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_device.hpp"
#include "ba_triangulate.hpp"

namespace pcs {

// camera row: [R_e | t_e] world -> camera rows of a 3 x 4 (12) | position -R_e^T t_e (3) | .. | intr at 22 as undistort5 reads it
// (fx cx fy cy k0 k1 p0 p1 k2) | V = R_new^T row-major (9) | K_new fx cx fy cy (4)
constexpr int IMAP_CAM_STRIDE = 48;
constexpr int IMAP_EXT = 0, IMAP_POS = 12, IMAP_INTR = 22, IMAP_VIEW = 32, IMAP_KNEW = 41;
static_assert(IMAP_INTR == 22 && IMAP_CAM_STRIDE >= TRI_CAM_STRIDE, "undistort5 reads the intrinsics at 22 of a camera row");

constexpr int IMAP_PX = 4;                    // destination pixels per lane
constexpr int IMAP_TILE_X = 32, IMAP_TILE_Y = 8;   // lanes x rows of a workgroup
constexpr int IMAP_MODE_UNDISTORT = 0, IMAP_MODE_DISTORT = 1, IMAP_MODE_RAY = 2;
constexpr int IMAP_NORMALISED = 1, IMAP_WORLD = 2, IMAP_NO_DISTORT = 4;
constexpr int IMAP_NEAREST = 0, IMAP_BILINEAR = 1, IMAP_BICUBIC = 2;
constexpr int IMAP_COORD_FUSED = 0, IMAP_COORD_MAP_F32 = 1, IMAP_COORD_MAP_F64 = 2;

// detected pixel -> undistorted pixel: nb_undistort_prealloc's fixed point.  Five steps are undistort5 itself; another count runs the
// same step `iters` times (0: the pixel unchanged).
__device__ __forceinline__ void imap_undistort(const double u, const double v, const double *__restrict__ ct, const int iters, double &uo, double &vo) {
    if (iters == 5) {
        undistort5(u, v, ct, uo, vo);
        return;
    }
    const double fx = ct[22], cx = ct[23], fy = ct[24], cy = ct[25];
    const double k0 = ct[26], k1 = ct[27], p0 = ct[28], p1 = ct[29], k2 = ct[30];
    const double x0 = (u - cx) / fx, y0 = (v - cy) / fy;
    double x = x0, y = y0;
    for (int it = 0; it < iters; ++it) {
        const double r2 = x * x + y * y;
        const double k_inv = 1.0 / (1.0 + k0 * r2 + k1 * (r2 * r2) + k2 * (r2 * r2 * r2));
        const double xD = 2.0 * p0 * x * y + p1 * (r2 + 2.0 * (x * x));
        const double yD = p0 * (r2 + 2.0 * (y * y)) + 2.0 * p1 * x * y;
        x = (x0 - xD) * k_inv;
        y = (y0 - yD) * k_inv;
    }
    uo = x * fx + cx;
    vo = y * fy + cy;
}

// The camera slab eval_detection reads (ba_device.hpp: intr 9 | R 9 | t 3), with R the view rotation V (or the identity) and t = 0.
__device__ __forceinline__ void imap_slab(const double *__restrict__ ct, const bool view, double (&cs)[21]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) cs[i] = ct[IMAP_INTR + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) cs[CAM_R + i] = view ? ct[IMAP_VIEW + i] : ((i & 3) == 0 ? 1.0 : 0.0);
    cs[CAM_T] = cs[CAM_T + 1] = cs[CAM_T + 2] = 0.0;
}

// (x, y, z) in the frame the slab's R turns into the source camera -> the source pixel, by the forward model of the engine
__device__ __forceinline__ void imap_project(const double (&cs)[21], const double x, const double y, const double z, double &u, double &v) {
    double J[2 * chain_P(CHAIN_FREE)];   // JAC = false: never written
    eval_detection<CHAIN_FREE, double, false>((const double *)cs, (const double *)nullptr, x, y, z, u, v, J);
}

// destination pixel (u, v) of the view -> source pixel; NaN where the point lies behind the source camera (Z <= 0)
__device__ __forceinline__ void imap_source_coord(const double *__restrict__ ct, const double (&cs)[21], const double u, const double v, double &sx, double &sy) {
    const double xn = (u - ct[IMAP_KNEW + 1]) / ct[IMAP_KNEW + 0], yn = (v - ct[IMAP_KNEW + 3]) / ct[IMAP_KNEW + 2];
    const double z = cs[CAM_R + 6] * xn + cs[CAM_R + 7] * yn + cs[CAM_R + 8];
    imap_project(cs, xn, yn, 1.0, sx, sy);
    if (!(z > 0.0)) sx = sy = __builtin_nan("");
}

// pixel -> ray (vector_cam_points / sensor_map): undistort, K^-1, linear (z = 1) or unit length, camera frame or world
__device__ __forceinline__ void imap_ray(const double *__restrict__ ct, double u, double v, const int flags, const int iters, double (&r)[3]) {
    if (!(flags & IMAP_NO_DISTORT)) imap_undistort(u, v, ct, iters, u, v);
    double x = (u - ct[23]) / ct[22], y = (v - ct[25]) / ct[24], z = 1.0;
    if (flags & IMAP_NORMALISED) {
        const double inv = 1.0 / sqrt(x * x + y * y + 1.0);
        x *= inv, y *= inv, z = inv;
    }
    if (flags & IMAP_WORLD) {   // R_e^T: camera -> world, a direction
        r[0] = ct[0] * x + ct[4] * y + ct[8] * z;
        r[1] = ct[1] * x + ct[5] * y + ct[9] * z;
        r[2] = ct[2] * x + ct[6] * y + ct[10] * z;
    } else {
        r[0] = x, r[1] = y, r[2] = z;
    }
}

__global__ __launch_bounds__(256) void imap_points_kernel(const double *__restrict__ tab, const int n_cams, const int mode, const int64_t n, const int32_t *__restrict__ cam,
                                                          const int cam_all, const double2 *__restrict__ in, const int iters, const int flags, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = cam ? cam[i] : cam_all;
    const int width = mode == IMAP_MODE_RAY ? 3 : 2;
    double r[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    if (c >= 0 && c < n_cams) {   // a camera outside the table: NaN, nothing is read
        const double *ct = tab + (int64_t)c * IMAP_CAM_STRIDE;
        const double2 p = in[i];
        if (mode == IMAP_MODE_UNDISTORT) {
            imap_undistort(p.x, p.y, ct, iters, r[0], r[1]);
        } else if (mode == IMAP_MODE_DISTORT) {
            double cs[21];
            imap_slab(ct, false, cs);
            imap_project(cs, (p.x - ct[23]) / ct[22], (p.y - ct[25]) / ct[24], 1.0, r[0], r[1]);
        } else {
            imap_ray(ct, p.x, p.y, flags, iters, r);
        }
    }
    double *o = out + i * width;
    o[0] = r[0], o[1] = r[1];
    if (width == 3) o[2] = r[2];
}

template <class OutT>
__global__ __launch_bounds__(256) void imap_raymap_kernel(const double *__restrict__ tab, const int cam, const int W, const int H, const int flags, const int iters,
                                                          const void *__restrict__ depth, const int depth_f32, OutT *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)W * H) return;
    const double *ct = tab + (int64_t)cam * IMAP_CAM_STRIDE;
    const int x = (int)(i % W), y = (int)(i / W);
    double r[3];
    imap_ray(ct, (double)x, (double)y, flags, iters, r);
    if (depth) {   // im_to_world_ray(depth_im=): position + ray * depth; a depth that is no number gives no point
        const double d = depth_f32 ? (double)static_cast<const float *>(depth)[i] : static_cast<const double *>(depth)[i];
        const bool ok = (d - d) == 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = ok ? ((flags & IMAP_WORLD) ? ct[IMAP_POS + k] : 0.0) + r[k] * d : __builtin_nan("");
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[i * 3 + k] = (OutT)r[k];
}

template <class OutT>
__global__ __launch_bounds__(256) void imap_build_maps_kernel(const double *__restrict__ tab, const int cam, const int Wd, const int Hd, OutT *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, plane = (int64_t)Wd * Hd;
    if (i >= plane) return;
    const double *ct = tab + (int64_t)cam * IMAP_CAM_STRIDE;
    double cs[21], sx, sy;
    imap_slab(ct, true, cs);
    imap_source_coord(ct, cs, (double)(i % Wd), (double)(i / Wd), sx, sy);
    out[i] = (OutT)sx;
    out[plane + i] = (OutT)sy;
}

struct ImapBorder { double v[4]; };

// one tap: the source value, or the border value outside the source
template <class T, int C>
__device__ __forceinline__ bool imap_tap(const char *__restrict__ img, const int Ws, const int Hs, const int64_t pitch, const int x, const int y, const ImapBorder &border,
                                         double (&t)[C]) {
    const bool inside = (unsigned)x < (unsigned)Ws && (unsigned)y < (unsigned)Hs;
    if (inside) {
        const T *p = reinterpret_cast<const T *>(img + (int64_t)y * pitch) + (int64_t)x * C;
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = (double)p[c];
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] = border.v[c];
    }
    return inside;
}

// Keys' cubic convolution weights, a = -0.75, of the taps at -1, 0, 1, 2 around a fraction t in [0, 1) (cv2's interpolateCubic)
__device__ __forceinline__ void imap_cubic_weights(const double t, double (&w)[4]) {
    constexpr double A = -0.75;
    w[0] = ((A * (t + 1.0) - 5.0 * A) * (t + 1.0) + 8.0 * A) * (t + 1.0) - 4.0 * A;
    w[1] = ((A + 2.0) * t - (A + 3.0)) * t * t + 1.0;
    w[2] = ((A + 2.0) * (1.0 - t) - (A + 3.0)) * (1.0 - t) * (1.0 - t) + 1.0;
    w[3] = 1.0 - w[0] - w[1] - w[2];
}

// The one sampling routine: out[C] in FP64 and whether every tap lay inside.
template <class T, int C, int INTERP>
__device__ __forceinline__ bool imap_sample(const char *__restrict__ img, const int Ws, const int Hs, const int64_t pitch, const double sx, const double sy,
                                            const ImapBorder &border, double (&out)[C]) {
    // no tap can be inside (this also takes NaN and whatever would not fit an int)
    if (!(sx >= -3.0 && sx <= (double)Ws + 2.0 && sy >= -3.0 && sy <= (double)Hs + 2.0)) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = border.v[c];
        return false;
    }
    bool all = true, any = false;
    if constexpr (INTERP == IMAP_NEAREST) {
        all = any = imap_tap<T, C>(img, Ws, Hs, pitch, (int)rint(sx), (int)rint(sy), border, out);
    } else if constexpr (INTERP == IMAP_BILINEAR) {
        const double xf = floor(sx), yf = floor(sy), fx = sx - xf, fy = sy - yf;
        const int x0 = (int)xf, y0 = (int)yf;
        double row[2][C];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            double t0[C], t1[C];
            const bool i0 = imap_tap<T, C>(img, Ws, Hs, pitch, x0, y0 + j, border, t0), i1 = imap_tap<T, C>(img, Ws, Hs, pitch, x0 + 1, y0 + j, border, t1);
            all = all && i0 && i1, any = any || i0 || i1;
#pragma unroll
            for (int c = 0; c < C; ++c) row[j][c] = t0[c] * (1.0 - fx) + t1[c] * fx;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = row[0][c] * (1.0 - fy) + row[1][c] * fy;
    } else {
        const double xf = floor(sx), yf = floor(sy);
        const int x0 = (int)xf, y0 = (int)yf;
        double wx[4], wy[4];
        imap_cubic_weights(sx - xf, wx);
        imap_cubic_weights(sy - yf, wy);
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double row[C];
#pragma unroll
            for (int c = 0; c < C; ++c) row[c] = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double t[C];
                const bool in = imap_tap<T, C>(img, Ws, Hs, pitch, x0 - 1 + i, y0 - 1 + j, border, t);
                all = all && in, any = any || in;
#pragma unroll
                for (int c = 0; c < C; ++c) row[c] += wx[i] * t[c];
            }
#pragma unroll
            for (int c = 0; c < C; ++c) out[c] += wy[j] * row[c];
        }
    }
    if (!any) {
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = border.v[c];
    }
    return all;
}

__device__ __forceinline__ uint8_t imap_store_value(const double v, uint8_t) { return (uint8_t)fmin(fmax(rint(v), 0.0), 255.0); }   // NaN -> 0
__device__ __forceinline__ float imap_store_value(const double v, float) { return (float)v; }

struct ImapRemapArgs {
    const void *src;        // (n_img, Hs, src_pitch bytes)
    void *dst;              // (n_img, Hd, dst_pitch bytes)
    uint8_t *valid;         // (n_img, Hd, Wd) or NULL
    const void *map;        // (n_maps, 2, Hd, Wd) float or double; unused when fused
    const int32_t *cams;    // (n_img): the camera (fused) or the map (mapped) of every image, range-checked by the host
    const double *tab;
    int coord, Ws, Hs, Wd, Hd;
    int64_t src_pitch, dst_pitch;
    ImapBorder border;
};

template <class T, int C, int INTERP>
__global__ __launch_bounds__(IMAP_TILE_X * IMAP_TILE_Y) void imap_remap_kernel(const ImapRemapArgs a) {
    const int img = blockIdx.z, y = blockIdx.y * IMAP_TILE_Y + threadIdx.y, xq = (blockIdx.x * IMAP_TILE_X + threadIdx.x) * IMAP_PX;
    if (y >= a.Hd || xq >= a.Wd) return;
    const int cam = a.cams[img];
    const double *ct = a.tab + (int64_t)cam * IMAP_CAM_STRIDE;
    double cs[21];
    if (a.coord == IMAP_COORD_FUSED) imap_slab(ct, true, cs);
    const char *simg = static_cast<const char *>(a.src) + (int64_t)img * a.Hs * a.src_pitch;
    const int64_t plane = (int64_t)a.Wd * a.Hd, mrow = (int64_t)cam * 2 * plane + (int64_t)y * a.Wd;
    const int n = min(IMAP_PX, a.Wd - xq);
    T res[IMAP_PX * C];
    uint8_t ok[IMAP_PX];
#pragma unroll
    for (int k = 0; k < IMAP_PX; ++k) {
        double sx, sy, val[C];
        if (k < n) {
            if (a.coord == IMAP_COORD_FUSED) {
                imap_source_coord(ct, cs, (double)(xq + k), (double)y, sx, sy);
            } else if (a.coord == IMAP_COORD_MAP_F32) {
                const float *m = static_cast<const float *>(a.map) + mrow + xq + k;
                sx = (double)m[0], sy = (double)m[plane];
            } else {
                const double *m = static_cast<const double *>(a.map) + mrow + xq + k;
                sx = m[0], sy = m[plane];
            }
            ok[k] = imap_sample<T, C, INTERP>(simg, a.Ws, a.Hs, a.src_pitch, sx, sy, a.border, val) ? 1 : 0;
        } else {
            ok[k] = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) val[c] = 0.0;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) res[k * C + c] = imap_store_value(val[c], T());
    }
    char *drow = static_cast<char *>(a.dst) + ((int64_t)img * a.Hd + y) * a.dst_pitch + (int64_t)xq * C * sizeof(T);
    constexpr int BYTES = IMAP_PX * C * sizeof(T);
    constexpr int ALIGN = sizeof(T) == 1 ? 4 : 16;   // 8-bit: whole dwords; float: 16-byte stores
    if (n == IMAP_PX && (reinterpret_cast<uintptr_t>(drow) & (ALIGN - 1)) == 0) {
        if constexpr (sizeof(T) == 1) {
            uint32_t *d = reinterpret_cast<uint32_t *>(drow);
#pragma unroll
            for (int w = 0; w < BYTES / 4; ++w)
                d[w] = (uint32_t)res[4 * w] | ((uint32_t)res[4 * w + 1] << 8) | ((uint32_t)res[4 * w + 2] << 16) | ((uint32_t)res[4 * w + 3] << 24);
        } else {
            float4 *d = reinterpret_cast<float4 *>(drow);
#pragma unroll
            for (int w = 0; w < BYTES / 16; ++w) d[w] = make_float4(res[4 * w], res[4 * w + 1], res[4 * w + 2], res[4 * w + 3]);
        }
    } else {   // the row tail, or a row that does not start on the store's alignment
        T *d = reinterpret_cast<T *>(drow);
#pragma unroll
        for (int k = 0; k < IMAP_PX; ++k)
            if (k < n) {
#pragma unroll
                for (int c = 0; c < C; ++c) d[k * C + c] = res[k * C + c];
            }
    }
    if (a.valid) {
        uint8_t *vrow = a.valid + ((int64_t)img * a.Hd + y) * a.Wd + xq;
        if (n == IMAP_PX && (reinterpret_cast<uintptr_t>(vrow) & 3) == 0) {
            *reinterpret_cast<uint32_t *>(vrow) = (uint32_t)ok[0] | ((uint32_t)ok[1] << 8) | ((uint32_t)ok[2] << 16) | ((uint32_t)ok[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < IMAP_PX; ++k)
                if (k < n) vrow[k] = ok[k];
        }
    }
}

}  // namespace pcs
