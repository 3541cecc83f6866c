// ba_tsdf.hpp — depth maps to a surface: the TSDF volume and the surface-nets extraction (include/pcs_hip.h, "TSDF volume and surface
// extraction"; host side: pcs_tsdf.inc).
//
// tsdf_integrate_kernel: one thread per node, x fastest across lanes, a workgroup a TSDF_TX x TSDF_TY brick of ONE z-slab.  The loop
// over the view list sits inside the thread with the running sum and weight in registers, so the volume is read and written once per
// call, not once per view.  The view's 16 doubles and the list entry are the same in every lane (wave-uniform addresses, as in
// fuse_check_kernel): a loop over the list, nothing per lane indexed at run time.  The transform and the projection are ba_fusion.hpp's
// (fuse_load_view, fuse_to_view, fuse_project): the written order of operations is the same.  fuse_partner is NOT reused: it does not
// hand back Y_z, which the signed distance needs, so tsdf_partner below is its body with Y_z returned.
//
// The extraction runs per cell and per grid edge; the stable ordered compaction in between is the project's own (stereo_count_kernel /
// stereo_scan_kernel of ba_stereo.hpp, unchanged): the cell flags are nz - 1 "views" of (ny - 1)(nx - 1) pixels, the quad flags 3 nz of
// ny nx.
//   tsdf_classify_kernel    an ACTIVE flag per cell
//   tsdf_number_kernel      flags + block offsets -> the dense int32 cell -> vertex number map (-1: no vertex), the hand-over to the quads
//   tsdf_quad_flag_kernel   one flag per (axis, node): the edge emits a quad
//   tsdf_vertex_kernel      the vertex of every active cell at its number
//   tsdf_quad_write_kernel  the four vertex numbers of every flagged edge at its rank
// No atomics; every output position is the rule's.  Contraction is off in every function: plain IEEE-754 double operations in the order
// written.  Every node, cell and byte index is int64_t.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_fusion.hpp"
#include "ba_stereo.hpp"

namespace pcs {

constexpr int TSDF_TX = 32, TSDF_TY = 8;   // the brick: a wave is two rows of 32 nodes
constexpr int TSDF_MAX_DIM = 1024;
constexpr int TSDF_MAX_WEIGHT = 65535;

struct TsdfGrid {
    double o[3], s;
    int nx, ny, nz;
};

struct TsdfIntegrateArgs {
    const double *views;    // (V, 16): the table of pcs_fuse_set_views
    const int32_t *list;    // (n_list) or NULL: views 0 .. n_list - 1
    int n_list;
    const void *depth;      // (V, H, W) float or double
    int W, H;
    TsdfGrid g;
    double trunc;
    void *sum;              // (nz, ny, nx) float or double
    uint16_t *weight;
};

// fuse_partner with Y_z handed back: q = (floor(u + 0.5), floor(w + 0.5)); false behind the view or outside the image.  A NaN fails every
// comparison, and q is converted only once it is known to lie inside.
__device__ __forceinline__ bool tsdf_partner(const FuseView &v, double X0, double X1, double X2, int W, int H, int &qx, int &qy, double &Yz) {
#pragma clang fp contract(off)
    double Y0, Y1, Y2, u, w;
    fuse_to_view(v, X0, X1, X2, Y0, Y1, Y2);
    Yz = Y2;
    if (!(Y2 > 0.0)) return false;
    fuse_project(v, Y0, Y1, Y2, u, w);
    const double fu = floor(u + 0.5), fw = floor(w + 0.5);
    if (!(fu >= 0.0 && fu < (double)W && fw >= 0.0 && fw < (double)H)) return false;
    qx = (int)fu, qy = (int)fw;
    return true;
}

template <class T, class S>
__global__ __launch_bounds__(TSDF_TX *TSDF_TY) void tsdf_integrate_kernel(const TsdfIntegrateArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * TSDF_TX + threadIdx.x, j = blockIdx.y * TSDF_TY + threadIdx.y, k = blockIdx.z;
    if (i >= a.g.nx || j >= a.g.ny) return;
    const int64_t n = ((int64_t)k * a.g.ny + j) * a.g.nx + i, HW = (int64_t)a.H * a.W;
    const T *__restrict__ D = static_cast<const T *>(a.depth);
    S *__restrict__ sum = static_cast<S *>(a.sum);
    const double X0 = a.g.o[0] + a.g.s * (double)i, X1 = a.g.o[1] + a.g.s * (double)j, X2 = a.g.o[2] + a.g.s * (double)k;
    double acc = (double)sum[n];
    unsigned wgt = a.weight[n];
    for (int l = 0; l < a.n_list; ++l) {   // the same trip count and the same view in every lane
        const int v = a.list ? a.list[l] : l;
        const FuseView vw = fuse_load_view(a.views, v);
        int qx = 0, qy = 0;
        double Yz;
        bool ok = tsdf_partner(vw, X0, X1, X2, a.W, a.H, qx, qy, Yz);
        double d = 0.0;
        if (ok) d = (double)D[(int64_t)v * HW + (int64_t)qy * a.W + qx];
        ok = ok && fuse_depth_valid(d);
        const double sdf = d - Yz;
        ok = ok && sdf >= -a.trunc;
        const double r = sdf / a.trunc;
        if (ok) {
            acc = acc + (r < 1.0 ? r : 1.0);
            wgt += 1u;
        }
    }
    sum[n] = (S)acc;
    a.weight[n] = (uint16_t)wgt;
}

struct TsdfExtractArgs {
    const void *sum;
    const uint16_t *weight;
    TsdfGrid g;
    int min_weight, nblk;      // nblk: 256-pixel blocks per "view" of the compaction this kernel reads or feeds
    uint8_t *flag;             // cells, or 3 x nodes
    const int64_t *off;        // block offsets of the scan
    int32_t *map;              // cells
    void *vertices;            // (n_v, 3)
    int32_t *quads;            // (n_q, 4)
};

// OBSERVED, and the value D = double(sum) / double(weight); `inside` iff observed and D < 0
template <class S>
__device__ __forceinline__ bool tsdf_node(const TsdfExtractArgs &a, int64_t n, double &Dn, bool &inside) {
#pragma clang fp contract(off)
    const unsigned w = a.weight[n];
    const bool obs = w >= (unsigned)a.min_weight;
    Dn = (double)static_cast<const S *>(a.sum)[n] / (double)w;
    inside = obs && Dn < 0.0;
    return obs;
}

// the eight corners of cell (i, j, k): all observed?  D and INSIDE per corner
template <class S>
__device__ __forceinline__ bool tsdf_corners(const TsdfExtractArgs &a, int i, int j, int k, double (&Dc)[8], bool (&in)[8]) {
    bool all = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t n = ((int64_t)(k + (c >> 2 & 1)) * a.g.ny + (j + (c >> 1 & 1))) * a.g.nx + (i + (c & 1));
        all = tsdf_node<S>(a, n, Dc[c], in[c]) && all;
    }
    return all;
}

// One thread per cell, blockIdx.y the cell slab k: the layout stereo_count_kernel reads.
template <class S>
__global__ __launch_bounds__(STEREO_PIX_PER_BLOCK) void tsdf_classify_kernel(const TsdfExtractArgs a) {
    const int cx = a.g.nx - 1, cy = a.g.ny - 1, k = blockIdx.y;
    const int64_t HW = (int64_t)cx * cy, p = (int64_t)blockIdx.x * STEREO_PIX_PER_BLOCK + threadIdx.x;
    if (p >= HW) return;
    const int j = (int)(p / cx), i = (int)(p - (int64_t)j * cx);
    double Dc[8];
    bool in[8];
    const bool all = tsdf_corners<S>(a, i, j, k, Dc, in);
    int n_in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) n_in += in[c] ? 1 : 0;
    a.flag[(int64_t)k * HW + p] = (uint8_t)(all && n_in > 0 && n_in < 8);
}

// map[cell] = its vertex number, the rank of its flag in cell order (stereo_scatter_kernel's ranking), or -1
__global__ __launch_bounds__(STEREO_PIX_PER_BLOCK) void tsdf_number_kernel(const TsdfExtractArgs a) {
    __shared__ int wave_cnt[STEREO_PIX_PER_BLOCK / 64];
    const int64_t HW = (int64_t)(a.g.nx - 1) * (a.g.ny - 1), p = (int64_t)blockIdx.x * STEREO_PIX_PER_BLOCK + threadIdx.x;
    const int k = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)k * HW + p;
    const bool m = p < HW && a.flag[g] != 0;
    const unsigned long long b = __ballot(m);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    if (p >= HW) return;
    int64_t dst = a.off[(int64_t)k * a.nblk + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) dst += wave_cnt[w];
    a.map[g] = m ? (int32_t)dst : -1;
}

// one crossing of the vertex: edge (A, B) of the cell along `axis`, added when its ends differ in INSIDE
template <int A, int B>
__device__ __forceinline__ void tsdf_edge(const double (&Dc)[8], const bool (&in)[8], double &s0, double &s1, double &s2, int &cnt) {
#pragma clang fp contract(off)
    constexpr int axis = B - A == 1 ? 0 : B - A == 2 ? 1 : 2;
    if (in[A] == in[B]) return;
    const double t = Dc[A] / (Dc[A] - Dc[B]);
    s0 = s0 + (axis == 0 ? t : (double)(A & 1));
    s1 = s1 + (axis == 1 ? t : (double)(A >> 1 & 1));
    s2 = s2 + (axis == 2 ? t : (double)(A >> 2 & 1));
    cnt += 1;
}

template <class TV, class S>
__global__ __launch_bounds__(STEREO_PIX_PER_BLOCK) void tsdf_vertex_kernel(const TsdfExtractArgs a) {
#pragma clang fp contract(off)
    const int cx = a.g.nx - 1, cy = a.g.ny - 1, k = blockIdx.y;
    const int64_t HW = (int64_t)cx * cy, p = (int64_t)blockIdx.x * STEREO_PIX_PER_BLOCK + threadIdx.x;
    if (p >= HW) return;
    const int32_t num = a.map[(int64_t)k * HW + p];
    if (num < 0) return;
    const int j = (int)(p / cx), i = (int)(p - (int64_t)j * cx);
    double Dc[8];
    bool in[8];
    (void)tsdf_corners<S>(a, i, j, k, Dc, in);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int cnt = 0;
    tsdf_edge<0, 1>(Dc, in, s0, s1, s2, cnt), tsdf_edge<0, 2>(Dc, in, s0, s1, s2, cnt), tsdf_edge<0, 4>(Dc, in, s0, s1, s2, cnt);
    tsdf_edge<1, 3>(Dc, in, s0, s1, s2, cnt), tsdf_edge<1, 5>(Dc, in, s0, s1, s2, cnt), tsdf_edge<2, 3>(Dc, in, s0, s1, s2, cnt);
    tsdf_edge<2, 6>(Dc, in, s0, s1, s2, cnt), tsdf_edge<3, 7>(Dc, in, s0, s1, s2, cnt), tsdf_edge<4, 5>(Dc, in, s0, s1, s2, cnt);
    tsdf_edge<4, 6>(Dc, in, s0, s1, s2, cnt), tsdf_edge<5, 7>(Dc, in, s0, s1, s2, cnt), tsdf_edge<6, 7>(Dc, in, s0, s1, s2, cnt);
    const double m = (double)cnt;
    const double x = a.g.o[0] + a.g.s * ((double)i + s0 / m), y = a.g.o[1] + a.g.s * ((double)j + s1 / m), z = a.g.o[2] + a.g.s * ((double)k + s2 / m);
    TV *o = static_cast<TV *>(a.vertices) + 3 * (int64_t)num;
    o[0] = (TV)x, o[1] = (TV)y, o[2] = (TV)z;
}

// The grid edge from node n = (i, j, k) along axis A = blockIdx.y / nz: does it emit a quad, and with which four vertex numbers?  The
// cells around it are gathered only once their coordinates are known to lie inside the cell grid.
template <class S>
__device__ __forceinline__ bool tsdf_quad(const TsdfExtractArgs &a, int A, int i, int j, int k, int32_t (&id)[4]) {
    // (axis A, U, V) = (x, y, z), (y, z, x), (z, x, y), picked with selects: A is the same in every lane, and nothing is indexed at run time
    const int cx = a.g.nx - 1, cy = a.g.ny - 1;
    const int nA = A == 0 ? i : A == 1 ? j : k, dA = A == 0 ? a.g.nx : A == 1 ? a.g.ny : a.g.nz;
    const int nU = A == 0 ? j : A == 1 ? k : i, dU = A == 0 ? a.g.ny : A == 1 ? a.g.nz : a.g.nx;
    const int nV = A == 0 ? k : A == 1 ? i : j, dV = A == 0 ? a.g.nz : A == 1 ? a.g.nx : a.g.ny;
    if (nA + 1 >= dA) return false;
    const int64_t sx = 1, sy = a.g.nx, sz = (int64_t)a.g.nx * a.g.ny, csx = 1, csy = cx, csz = (int64_t)cx * cy;
    const int64_t n = ((int64_t)k * a.g.ny + j) * a.g.nx + i;
    double Da, Db;
    bool ia, ib;
    const bool oa = tsdf_node<S>(a, n, Da, ia), ob = tsdf_node<S>(a, n + (A == 0 ? sx : A == 1 ? sy : sz), Db, ib);
    if (!(oa && ob) || ia == ib) return false;
    if (nU < 1 || nU > dU - 2 || nV < 1 || nV > dV - 2) return false;   // the four cells exist
    const int64_t cU = A == 0 ? csy : A == 1 ? csz : csx, cV = A == 0 ? csz : A == 1 ? csx : csy;
    const int64_t c = ((int64_t)k * cy + j) * cx + i;
    const int32_t v0 = a.map[c - cU - cV], v1 = a.map[c - cV], v2 = a.map[c], v3 = a.map[c - cU];
    if (v0 < 0 || v1 < 0 || v2 < 0 || v3 < 0) return false;
    id[0] = ia ? v0 : v3, id[1] = ia ? v1 : v2, id[2] = ia ? v2 : v1, id[3] = ia ? v3 : v0;
    return true;
}

// One thread per (axis, node); blockIdx.y = A nz + k: the 3 nz "views" of ny nx pixels.
template <class S>
__global__ __launch_bounds__(STEREO_PIX_PER_BLOCK) void tsdf_quad_flag_kernel(const TsdfExtractArgs a) {
    const int64_t HW = (int64_t)a.g.nx * a.g.ny, p = (int64_t)blockIdx.x * STEREO_PIX_PER_BLOCK + threadIdx.x;
    if (p >= HW) return;
    const int A = blockIdx.y / a.g.nz, k = blockIdx.y - A * a.g.nz;
    const int j = (int)(p / a.g.nx), i = (int)(p - (int64_t)j * a.g.nx);
    int32_t id[4];
    a.flag[(int64_t)blockIdx.y * HW + p] = (uint8_t)tsdf_quad<S>(a, A, i, j, k, id);
}

template <class S>
__global__ __launch_bounds__(STEREO_PIX_PER_BLOCK) void tsdf_quad_write_kernel(const TsdfExtractArgs a) {
    __shared__ int wave_cnt[STEREO_PIX_PER_BLOCK / 64];
    const int64_t HW = (int64_t)a.g.nx * a.g.ny, p = (int64_t)blockIdx.x * STEREO_PIX_PER_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool m = p < HW && a.flag[(int64_t)blockIdx.y * HW + p] != 0;
    const unsigned long long b = __ballot(m);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    if (!m) return;
    int64_t dst = a.off[(int64_t)blockIdx.y * a.nblk + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) dst += wave_cnt[w];
    const int A = blockIdx.y / a.g.nz, k = blockIdx.y - A * a.g.nz;
    const int j = (int)(p / a.g.nx), i = (int)(p - (int64_t)j * a.g.nx);
    int32_t id[4] = {-1, -1, -1, -1};
    (void)tsdf_quad<S>(a, A, i, j, k, id);
    int32_t *o = a.quads + 4 * dst;
    o[0] = id[0], o[1] = id[1], o[2] = id[2], o[3] = id[3];
}

}  // namespace pcs
