// ba_stereo.hpp — dense stereo on a rectified pair: block matching, disparity to points, compaction.
//
// Reference: stereo_reconstruct / disparity_to_ptcld / depth_image_ptcloud_mask (reconstruction/reconstruction_utils.py:24-38, :110-137,
// :170-223), which lean on cv2.StereoBM and cv2.reprojectImageTo3D.  OpenCV's matcher is NOT reproduced bit for bit (its NORMALIZED_RESPONSE
// prefilter, SIMD rounding and dispDescale are its own); the rule here is all integers and stated in tests/stereo_reference.py.
//
// Kernels:
//   stereo_prefilter_kernel   the capped horizontal Sobel response of both images into two dense 8-bit planes (cap = 0: a copy).
//   stereo_fill_kernel        every pixel outside the strict rectangle: invalid disparity, cost -1, status bit 1.
//   stereo_match_kernel<RIGHT, K>   the matcher.  ONE WAVE per workgroup owns a tile of TW <= 64 anchor columns and a strip of SH rows and
//                             walks the strip downwards.  Lane t owns the K disparities dl = t + 64 k (Dpad = 64 K >= D).  LDS holds, per
//                             halo column xi (TW + 2r of them) and disparity, the COLUMN sum of absolute differences over the 2r + 1 rows of
//                             the current window (uint16: 31 * 255 fits): a row step adds the entering row and removes the leaving one, and
//                             the lane then slides along the row, adding the entering column sum and removing the leaving one.  Work per
//                             (pixel, disparity) is two absolute differences (v_sad_u8) and five LDS accesses whatever the window.  The
//                             cost of a pixel for all disparities therefore sits in the K registers of the 64 lanes at the moment the lane
//                             loop reaches it: the winner is a wave minimum over (cost << 10 | dl) (smallest cost, then smallest d), its
//                             neighbours are read from the lane that holds them, and the uniqueness rule is a second wave minimum with the
//                             winner's neighbourhood masked.  Nothing of the cost volume is ever stored.  Lane p keeps the results of
//                             pixel p of the row and finishes it (texture, left-right, validity, sub-pixel) with one coalesced store per row.
//                             RIGHT = true anchors in the right image (d_R for the left-right check, range clamped per pixel).
//   stereo_reproject_kernel   Q (x, y, disp / 16, 1), FP64, the reference's mask, optional rigid transform, per-block mask counts.
//   stereo_count_kernel / stereo_scan_kernel / stereo_scatter_kernel   stable compaction: counts per 256 pixels, one exclusive scan over
//                             all blocks of all pairs, ordered scatter.  No atomics anywhere: two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pcs {

constexpr int STEREO_MAX_DISP = 1024, STEREO_MAX_BLOCK = 31, STEREO_MAX_CAP = 63, STEREO_MAX_TW = 64, STEREO_MAX_K = 16;
constexpr int STEREO_NOT_STRICT = 1, STEREO_TEXTURE = 2, STEREO_UNIQUENESS = 4, STEREO_LEFT_RIGHT = 8, STEREO_VALIDITY = 16;
constexpr uint32_t STEREO_INF = 0xFFFFFFFFu;
constexpr int STEREO_NO_DR = -32768;      // d_R of a right pixel for which no disparity of the range is defined
constexpr int STEREO_PIX_PER_BLOCK = 256;   // reprojection / compaction: pixels per workgroup

// LDS of one matcher workgroup, in bytes: [column sums uint16 (TWH, Dpad)] [texture column sums uint16 (TWH)] [anchor rows, entering and
// leaving, uint8 (2, TWHp)] [other rows uint8 (2, SEGp)], TWH = TW + 2r halo columns, SEG = TWH + Dpad - 1.
__host__ __device__ inline int stereo_pad4(int v) { return (v + 3) & ~3; }
__host__ __device__ inline int64_t stereo_lds_bytes(int TW, int r, int Dpad) {
    const int TWH = TW + 2 * r;
    return (int64_t)2 * TWH * Dpad + 2 * stereo_pad4(TWH) + 2 * stereo_pad4(TWH) + 2 * stereo_pad4(TWH + Dpad - 1);
}

struct StereoMatchArgs {
    const uint8_t *PL, *PR;   // prefiltered planes (n, H, W), dense
    int W, H, dmin, D, r, TW, SH;
    int x_begin, x_end, y_begin, y_end;   // the anchor pixels of this launch (ends exclusive)
    int16_t *dR;                          // (n, H, W): written by RIGHT, read by the left pass when lr >= 0
    int cap, tex_thr, uniq, lr, inv;
    const uint8_t *vL, *vR;               // validity planes (n, H, W) or NULL
    int16_t *disp;
    int32_t *cost;     // or NULL
    uint8_t *status;   // or NULL
};

__global__ void stereo_prefilter_kernel(const uint8_t *L, const uint8_t *R, int64_t pitchL, int64_t pitchR, int W, int H, int cap, int n, uint8_t *PL, uint8_t *PR) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const bool right = (int)blockIdx.z >= n;
    const int64_t img = right ? (int)blockIdx.z - n : (int)blockIdx.z;
    const int64_t pitch = right ? pitchR : pitchL;
    const uint8_t *I = (right ? R : L) + img * H * pitch;
    uint8_t *P = (right ? PR : PL) + img * H * (int64_t)W;
    int v;
    if (cap == 0) {
        v = I[y * pitch + x];
    } else if (x == 0 || x == W - 1) {
        v = cap;
    } else {
        const uint8_t *r0 = I + (int64_t)max(y - 1, 0) * pitch, *r1 = I + (int64_t)y * pitch, *r2 = I + (int64_t)min(y + 1, H - 1) * pitch;
        const int g = ((int)r0[x + 1] - (int)r0[x - 1]) + 2 * ((int)r1[x + 1] - (int)r1[x - 1]) + ((int)r2[x + 1] - (int)r2[x - 1]);
        v = min(max(g, -cap), cap) + cap;
    }
    P[(int64_t)y * W + x] = (uint8_t)v;
}

// strict rectangle: [xs0, xs1) x [ys0, ys1) (empty when xs1 <= xs0 or ys1 <= ys0)
__global__ void stereo_fill_kernel(int W, int H, int xs0, int xs1, int ys0, int ys1, int inv, int16_t *disp, int32_t *cost, uint8_t *status) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    if (x >= xs0 && x < xs1 && y >= ys0 && y < ys1) return;
    const int64_t i = ((int64_t)blockIdx.z * H + y) * W + x;
    disp[i] = (int16_t)inv;
    if (cost) cost[i] = -1;
    if (status) status[i] = (uint8_t)STEREO_NOT_STRICT;
}

// minimum over the 64 lanes, the same value in every lane: four DPP steps inside each row of 16, then the four rows on the scalar unit
__device__ inline uint32_t stereo_wave_min(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));   // row_mirror
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return min(min(a, b), min(c, d));
}

// run[dl >> 6] of lane dl & 63 (dl wave-uniform).  Every register is read across and the choice is made on the scalar unit: choosing the
// register first is an indexed access to run[], which the compiler serves from scratch memory.
template <int K>
__device__ inline uint32_t stereo_cost_of(const uint32_t (&run)[K], int dl) {
    const int kq = dl >> 6, lane = __builtin_amdgcn_readfirstlane(dl & 63);
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t vk = (uint32_t)__builtin_amdgcn_readlane((int)run[k], lane);
        v = kq == k ? vk : v;
    }
    return v;
}

// the uniqueness rule on the winner's cost c and the smallest cost c2 at |d - d*| >= 2 (STEREO_INF: there is none)
__device__ inline bool stereo_not_unique(uint32_t c2, uint32_t c, int uniq) { return uniq > 0 && c2 != STEREO_INF && 100u * c2 <= (uint32_t)(100 + uniq) * c; }

// the sub-pixel offset in sixteenths from the costs m, c, p at d* - 1, d*, d* + 1 (dl = d* - min_disp): floor((32 (m - p) + den) / (2 den))
__device__ inline int stereo_subpixel(int dl, int D, int m, int c, int p) {
    int off = 0;
    if (dl > 0 && dl < D - 1) {
        const int den = 2 * (m + p - 2 * c);
        if (den != 0) {
            const int num = 32 * (m - p) + den, dd = 2 * den;   // dd > 0; floor division
            off = num / dd;
            if (num % dd != 0 && num < 0) --off;
        }
    }
    return off;
}

// the two lookups every finished pixel makes: the left-right check against d_R and the validity planes (row: offset of the pixel's row)
__device__ inline int stereo_lookup_bits(int d, int64_t at, int lr, const int16_t *dR, const uint8_t *vL, const uint8_t *vR) {
    int st = 0;
    if (lr >= 0 && abs(d - (int)dR[at - d]) > lr) st |= STEREO_LEFT_RIGHT;
    if (vL && (vL[at] == 0 || vR[at - d] == 0)) st |= STEREO_VALIDITY;
    return st;
}

template <bool RIGHT, int K>
__global__ __launch_bounds__(64) void stereo_match_kernel(const StereoMatchArgs a) {
    extern __shared__ __align__(16) unsigned char stereo_smem[];
    constexpr int Dpad = 64 * K;
    const int t = threadIdx.x, r = a.r, W = a.W, H = a.H, D = a.D;
    const int x0 = a.x_begin + (int)blockIdx.x * a.TW, x1 = min(x0 + a.TW, a.x_end);
    const int y0 = a.y_begin + (int)blockIdx.y * a.SH, y1 = min(y0 + a.SH, a.y_end);
    const int TWH = a.TW + 2 * r, TWHp = stereo_pad4(TWH), SEGp = stereo_pad4(TWH + Dpad - 1);
    const int ncol = (x1 - x0) + 2 * r, seg = ncol + Dpad - 1;
    uint16_t *colsum = reinterpret_cast<uint16_t *>(stereo_smem);
    uint16_t *tex = colsum + TWH * Dpad;
    uint8_t *sA = reinterpret_cast<uint8_t *>(tex + TWHp);
    uint8_t *sB = sA + 2 * TWHp;
    const int64_t plane = (int64_t)blockIdx.z * H * W;
    const uint8_t *A = (RIGHT ? a.PR : a.PL) + plane, *B = (RIGHT ? a.PL : a.PR) + plane;
    const int xa0 = x0 - r;                                                  // image column of halo column 0
    const int bs = RIGHT ? xa0 + a.dmin : xa0 - a.dmin - (Dpad - 1);         // image column of the other row's staged byte 0
    {
        uint32_t *z = reinterpret_cast<uint32_t *>(stereo_smem);
        const int words = (TWH * Dpad * 2 + TWHp * 2) / 4;
        for (int i = t; i < words; i += 64) z[i] = 0u;
    }
    __syncthreads();
    // what lane p knows about pixel p of the row being finished
    int my_dl = 0;
    uint32_t my_c = 0, my_m = 0, my_p = 0, my_c2 = STEREO_INF;
    for (int yn = y0 - r; yn <= y1 - 1 + r; ++yn) {
        const int yo = yn - (2 * r + 1), yc = yn - r;
        const bool has_old = yo >= y0 - r, out = yc >= y0;
        const uint8_t *An = A + (int64_t)yn * W, *Bn = B + (int64_t)yn * W;
        const uint8_t *Ao = A + (int64_t)(has_old ? yo : yn) * W, *Bo = B + (int64_t)(has_old ? yo : yn) * W;
        for (int i = t; i < ncol; i += 64) {
            const int xg = xa0 + i;
            const bool in = xg >= 0 && xg < W;
            const int vn = in ? An[xg] : 0, vo = in && has_old ? Ao[xg] : 0;
            sA[i] = (uint8_t)vn, sA[TWHp + i] = (uint8_t)vo;
            if (!RIGHT && a.cap > 0) tex[i] = (uint16_t)(tex[i] + abs(vn - a.cap) - (has_old ? abs(vo - a.cap) : 0));
        }
        for (int j = t; j < seg; j += 64) {
            const int xg = bs + j;
            const bool in = xg >= 0 && xg < W;
            sB[j] = in ? Bn[xg] : (uint8_t)0, sB[SEGp + j] = in && has_old ? Bo[xg] : (uint8_t)0;
        }
        __syncthreads();
        uint32_t run[K];
#pragma unroll
        for (int k = 0; k < K; ++k) run[k] = 0u;
        for (int xi = 0; xi < ncol; ++xi) {
            const uint32_t an = sA[xi], ao = sA[TWHp + xi];
            uint16_t *cs = colsum + xi * Dpad;
            const uint16_t *cs_out = colsum + (xi >= 2 * r + 1 ? xi - (2 * r + 1) : 0) * Dpad;
            const bool drop = xi >= 2 * r + 1;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int dl = t + 64 * k;
                const int bi = RIGHT ? xi + dl : xi + (Dpad - 1) - dl;
                const uint32_t bn = sB[bi], bo = sB[SEGp + bi];
                // column sum of (xi, dl): the entering row joins, the leaving row goes (a first window has no leaving row: both bytes are 0)
                const uint32_t c = __builtin_amdgcn_sad_u8(an, bn, (uint32_t)cs[dl]) - __builtin_amdgcn_sad_u8(ao, bo, 0u);
                cs[dl] = (uint16_t)c;
                if (out) {
                    run[k] += c;
                    if (drop) run[k] -= cs_out[dl];
                }
            }
            if (out && xi >= 2 * r) {
                const int px = xi - 2 * r, x = x0 + px;   // the pixel whose window is columns xi - 2r .. xi
                uint32_t best = STEREO_INF;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int dl = t + 64 * k;
                    bool ok = dl < D;
                    if (RIGHT) {
                        const int xo = x + a.dmin + dl;
                        ok = ok && xo >= r && xo <= W - 1 - r;
                    }
                    best = min(best, ok ? (run[k] << 10) | (uint32_t)dl : STEREO_INF);
                }
                best = stereo_wave_min(best);
                if (RIGHT) {
                    if (t == px) my_dl = best == STEREO_INF ? STEREO_NO_DR : a.dmin + (int)(best & 1023u);
                } else {
                    const int dls = (int)(best & 1023u);
                    const uint32_t C = best >> 10;
                    uint32_t m = 0u, p = 0u, c2 = STEREO_INF;
                    if (dls > 0 && dls < D - 1) m = stereo_cost_of<K>(run, dls - 1), p = stereo_cost_of<K>(run, dls + 1);
                    if (a.uniq > 0) {
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const int dl = t + 64 * k;
                            c2 = min(c2, dl < D && abs(dl - dls) >= 2 ? run[k] : STEREO_INF);
                        }
                        c2 = stereo_wave_min(c2);
                    }
                    if (t == px) my_dl = dls, my_c = C, my_m = m, my_p = p, my_c2 = c2;
                }
            }
        }
        if (out && t < x1 - x0) {
            const int x = x0 + t;
            const int64_t row = plane + (int64_t)yc * W;
            if (RIGHT) {
                a.dR[row + x] = (int16_t)my_dl;
            } else {
                const int d = a.dmin + my_dl;
                int st = 0;
                if (a.cap > 0) {
                    int s = 0;
                    for (int i = 0; i <= 2 * r; ++i) s += tex[t + i];
                    if (s < a.tex_thr) st |= STEREO_TEXTURE;
                }
                if (stereo_not_unique(my_c2, my_c, a.uniq)) st |= STEREO_UNIQUENESS;
                st |= stereo_lookup_bits(d, row + x, a.lr, a.dR, a.vL, a.vR);
                const int off = stereo_subpixel(my_dl, D, (int)my_m, (int)my_c, (int)my_p);
                a.disp[row + x] = (int16_t)(st ? a.inv : 16 * d + off);
                if (a.cost) a.cost[row + x] = (int32_t)my_c;
                if (a.status) a.status[row + x] = (uint8_t)st;
            }
        }
        __syncthreads();   // the next row step restages the rows and moves the texture sums
    }
}

struct StereoReprojArgs {
    const int16_t *disp;
    int W, H, invalid;
    const double *T;   // 12 doubles on the device or NULL
    const double *Q;   // (n_Q, 16) on the device
    int q_per_pair;
    double lo, hi;
    void *pts;
    int f32;
    uint8_t *mask;
    int32_t *blk;   // (n, nblk) mask counts per workgroup, or NULL
    int nblk;
};

__global__ __launch_bounds__(STEREO_PIX_PER_BLOCK) void stereo_reproject_kernel(const StereoReprojArgs a) {
    const int64_t HW = (int64_t)a.H * a.W, i = (int64_t)blockIdx.x * STEREO_PIX_PER_BLOCK + threadIdx.x;
    const int pair = blockIdx.y;
    int m = 0;
    if (i < HW) {
        const int64_t g = (int64_t)pair * HW + i;
        const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
        const int dq = a.disp[g];
        const double *Q = a.Q + (a.q_per_pair ? 16 * (int64_t)pair : 0);
        const double d = (double)dq / 16.0, xd = (double)x, yd = (double)y;
        const double X = Q[0] * xd + Q[1] * yd + Q[2] * d + Q[3], Y = Q[4] * xd + Q[5] * yd + Q[6] * d + Q[7];
        const double Z = Q[8] * xd + Q[9] * yd + Q[10] * d + Q[11], Wh = Q[12] * xd + Q[13] * yd + Q[14] * d + Q[15];
        double px = X / Wh, py = Y / Wh, pz = Z / Wh;
        m = dq != a.invalid && isfinite(px) && isfinite(py) && isfinite(pz) && pz >= a.lo && pz <= a.hi;
        if (!m) {
            px = py = pz = __builtin_nan("");
        } else if (a.T) {
            const double *T = a.T;
            const double qx = T[0] * px + T[1] * py + T[2] * pz + T[3], qy = T[4] * px + T[5] * py + T[6] * pz + T[7];
            const double qz = T[8] * px + T[9] * py + T[10] * pz + T[11];
            px = qx, py = qy, pz = qz;
        }
        if (a.f32) {
            float *o = static_cast<float *>(a.pts) + 3 * g;
            o[0] = (float)px, o[1] = (float)py, o[2] = (float)pz;
        } else {
            double *o = static_cast<double *>(a.pts) + 3 * g;
            o[0] = px, o[1] = py, o[2] = pz;
        }
        a.mask[g] = (uint8_t)m;
    }
    const int cnt = __syncthreads_count(m);
    if (a.blk && threadIdx.x == 0) a.blk[(int64_t)pair * a.nblk + blockIdx.x] = cnt;
}

__global__ __launch_bounds__(STEREO_PIX_PER_BLOCK) void stereo_count_kernel(const uint8_t *mask, int64_t HW, int nblk, int32_t *blk) {
    const int64_t i = (int64_t)blockIdx.x * STEREO_PIX_PER_BLOCK + threadIdx.x;
    const int m = i < HW && mask[(int64_t)blockIdx.y * HW + i] != 0;
    const int cnt = __syncthreads_count(m);
    if (threadIdx.x == 0) blk[(int64_t)blockIdx.y * nblk + blockIdx.x] = cnt;
}

// One workgroup of 1024: off[b] = the number of masked pixels in front of block b over ALL pairs (pair after pair), off[NB] the total;
// counts[p] the number of pair p.
__global__ __launch_bounds__(1024) void stereo_scan_kernel(const int32_t *blk, int64_t NB, int nblk, int n, int64_t *off, int64_t *counts) {
    __shared__ int64_t s[1024];
    __shared__ int64_t carry;
    const int t = threadIdx.x;
    if (t == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < NB; base += 1024) {
        const int64_t v = base + t < NB ? blk[base + t] : 0;
        s[t] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            const int64_t add = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        const int64_t incl = s[t], c = carry;
        if (base + t < NB) off[base + t] = c + incl - v;
        __syncthreads();
        if (t == 1023) carry = c + incl;
        __syncthreads();
    }
    if (t == 0) off[NB] = carry;
    __syncthreads();
    if (counts)
        for (int p = t; p < n; p += 1024) counts[p] = off[(int64_t)(p + 1) * nblk] - off[(int64_t)p * nblk];
}

struct StereoScatterArgs {
    const void *pts;
    int f32;
    const uint8_t *mask, *values;   // values (n, H, pitch) or NULL
    int64_t values_pitch;
    int W, H, nblk;
    const int64_t *off;
    void *out_pts;
    uint8_t *out_values;
};

__global__ __launch_bounds__(STEREO_PIX_PER_BLOCK) void stereo_scatter_kernel(const StereoScatterArgs a) {
    __shared__ int wave_cnt[STEREO_PIX_PER_BLOCK / 64];
    const int64_t HW = (int64_t)a.H * a.W, i = (int64_t)blockIdx.x * STEREO_PIX_PER_BLOCK + threadIdx.x;
    const int pair = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t g = (int64_t)pair * HW + i;
    const bool m = i < HW && a.mask[g] != 0;
    const unsigned long long b = __ballot(m);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    if (!m) return;
    int64_t dst = a.off[(int64_t)pair * a.nblk + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) dst += wave_cnt[w];
    if (a.f32) {
        const float *s = static_cast<const float *>(a.pts) + 3 * g;
        float *o = static_cast<float *>(a.out_pts) + 3 * dst;
        o[0] = s[0], o[1] = s[1], o[2] = s[2];
    } else {
        const double *s = static_cast<const double *>(a.pts) + 3 * g;
        double *o = static_cast<double *>(a.out_pts) + 3 * dst;
        o[0] = s[0], o[1] = s[1], o[2] = s[2];
    }
    if (a.values && a.out_values) {
        const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
        a.out_values[dst] = a.values[((int64_t)pair * a.H + y) * a.values_pitch + x];
    }
}

}  // namespace pcs
