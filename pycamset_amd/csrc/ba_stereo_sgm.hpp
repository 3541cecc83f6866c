// ba_stereo_sgm.hpp — semi-global matching on a rectified pair: census cost, 4 / 8-path aggregation, winner selection.
//
// Reference: matlab_stereo (reconstruction/reconstruction_utils.py:140-167), which starts a MATLAB engine and calls disparitySGM.  Neither
// MATLAB's nor OpenCV's semi-global matcher is reproduced bit for bit; the rule is all integers and stated in include/pcs_hip.h and in
// tests/sgm_reference.py.  Status bits, the int16 disparity, the right-anchored plane and the finish are those of ba_stereo.hpp.
//
// Kernels:
//   sgm_census_kernel         one 64-bit descriptor per pixel of both images: bit = (neighbour < centre), the window positions other than
//                             the centre in row-major order.  Pixels whose window leaves the image get 0 and are never read.
//   sgm_path_kernel<GROUP, K> ONE WAVE walks one line of the strict rectangle in one direction (GROUP: horizontal, vertical, diagonal; the
//                             sign is an argument).  Lane t owns the K CONTIGUOUS disparities K t .. K t + K - 1 and keeps L_r(p - r, .) of
//                             them in registers; the matching cost is one xor and one popcount per disparity on the two descriptors
//                             (sgm_cost), so the cost volume is never stored.  d - 1 / d + 1 are the neighbouring registers, and the two
//                             at the ends of a lane's run come from the neighbouring lanes by one DPP wave shift each: two cross-lane
//                             moves per step for every K (with d = t + 64 k it would be 2 K), and the K values of a lane are ONE 2 K-byte
//                             word of S, so a step moves one contiguous run of 2 Dpad bytes per wave.  min_j L_r is stereo_wave_min.
//                             The loads of a step (two descriptors, the old S) do not depend on the recurrence: they are issued
//                             SGM_PREFETCH steps ahead.  The first direction writes S, the others add to it; kernels are stream-ordered.
//   sgm_right_kernel          d_R from the diagonal of S.  A workgroup owns SGM_RIGHT_TX right pixels of a row and goes through the
//                             disparities SGM_RIGHT_DC at a time: the 2 SGM_RIGHT_DC-byte pieces of the runs of the left pixels that
//                             meet them are copied to LDS with coalesced loads (rows padded by one word: no bank conflict on the
//                             diagonal), and lane x2 then reads S(x2 + d, d) down its diagonal.
//   sgm_select_kernel<K>      one wave per 64 strict pixels of a row: per pixel the run of S, the winner and the uniqueness rule as two
//                             wave minima (as in stereo_match_kernel), then lane p finishes pixel p with the shared finish functions.
// No atomics and no scratch anywhere: every L_r term is an integer sum, so S has the same bits for any order of the directions.
#pragma once
#include "ba_stereo.hpp"

namespace pcs {

constexpr int SGM_MAX_DISP = 256, SGM_MAX_BITS = 64, SGM_MAX_P = 1023;
// L_r <= 64 + P2 <= 1087 and S <= 8 * 1087 = 8696 < 2^14: S is uint16 and (S << 10 | k) fits the 32-bit key of stereo_wave_min
constexpr int SGM_WAVES = 4;       // waves (lines) per workgroup of the path kernel
constexpr int SGM_PREFETCH = 4;    // steps the loads of the path kernel run ahead of the recurrence
constexpr int SGM_RIGHT_TX = 256, SGM_RIGHT_DC = 32, SGM_RIGHT_ROW = SGM_RIGHT_DC / 2 + 1;   // right kernel: pixels, disparities per pass, LDS words per row
constexpr uint32_t SGM_BIG = 0x0FFFFFFFu;   // L_r of a disparity outside the range: never the minimum, and BIG + P1 does not wrap
enum { SGM_HORIZONTAL = 0, SGM_VERTICAL = 1, SGM_DIAGONAL = 2 };

// The layout of S, shared by the host and every kernel: (pair, y, x, Dpad) uint16, d fastest.  K disparities per lane of a 64-lane wave.
__host__ __device__ inline int sgm_k(int D) { return D <= 64 ? 1 : D <= 128 ? 2 : 4; }
__host__ __device__ inline int sgm_dpad(int D) { return (D + 3) & ~3; }   // a multiple of every K: a lane's run is whole and 2 K-byte aligned
__host__ __device__ inline int64_t sgm_s_offset(int64_t pair, int y, int x, int W, int H, int Dpad) { return ((pair * H + y) * W + x) * Dpad; }
// bytes of workspace per pair: S and the two descriptor planes
__host__ __device__ inline int64_t sgm_pair_bytes(int W, int H, int Dpad) { return 2 * sgm_s_offset(1, 0, 0, W, H, Dpad) + 2 * 8 * (int64_t)H * W; }

struct SgmArgs {
    const uint64_t *cen;   // descriptors (2, nc, H, W): the nc left planes, then the nc right ones
    uint16_t *S;           // (nc, H, W, Dpad)
    int W, H, nc, dmin, D, Dpad;
    int xs0, xs1, ys0, ys1;   // the strict rectangle (ends exclusive)
    int p1, p2;
};

__global__ void sgm_census_kernel(const uint8_t *L, const uint8_t *R, int64_t pitchL, int64_t pitchR, int W, int H, int rw, int rh, int nc, uint64_t *cen) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const bool right = (int)blockIdx.z >= nc;
    const int64_t img = right ? (int)blockIdx.z - nc : (int)blockIdx.z;
    const int64_t pitch = right ? pitchR : pitchL;
    const uint8_t *I = (right ? R : L) + img * H * pitch;
    uint64_t bits = 0;
    if (x >= rw && x <= W - 1 - rw && y >= rh && y <= H - 1 - rh) {
        const int c = I[y * pitch + x];
        for (int j = -rh; j <= rh; ++j) {
            const uint8_t *row = I + (int64_t)(y + j) * pitch + x;
            for (int i = -rw; i <= rw; ++i)
                if (i != 0 || j != 0) bits = (bits << 1) | (uint64_t)((int)row[i] < c);
        }
    }
    cen[((int64_t)blockIdx.z * H + y) * W + x] = bits;
}

// The matching cost of the path kernel: another cost on two per-pixel words (Birchfield-Tomasi, absolute difference) replaces this.
__device__ inline uint32_t sgm_cost(uint64_t left, uint64_t right) { return (uint32_t)__popcll(left ^ right); }

// Line `line` of direction (dy, dx): its first pixel, where p - r is not strict, and its length.  false: no such line.
template <int GROUP>
__host__ __device__ inline bool sgm_line(int xs0, int xs1, int ys0, int ys1, int line, int dy, int dx, int &y, int &x, int &len) {
    const int Ws = xs1 - xs0, Hs = ys1 - ys0;
    const int yf = dy > 0 ? ys0 : ys1 - 1, xf = dx > 0 ? xs0 : xs1 - 1;   // the row and the column a path enters through
    if (GROUP == SGM_HORIZONTAL) {
        if (line >= Hs) return false;
        y = ys0 + line, x = xf, len = Ws;
    } else if (GROUP == SGM_VERTICAL) {
        if (line >= Ws) return false;
        y = yf, x = xs0 + line, len = Hs;
    } else {
        if (line >= Ws + Hs - 1) return false;
        if (line < Ws) y = yf, x = xs0 + line;   // the entry row, its corner included
        else y = yf + dy * (line - Ws + 1), x = xf;   // the rest of the entry column
        const int rows = dy > 0 ? ys1 - y : y - ys0 + 1, cols = dx > 0 ? xs1 - x : x - xs0 + 1;
        len = rows < cols ? rows : cols;
    }
    return true;
}
__host__ __device__ inline int sgm_line_count(int group, int Ws, int Hs) { return group == SGM_HORIZONTAL ? Hs : group == SGM_VERTICAL ? Ws : Ws + Hs - 1; }

// The K uint16 of one lane as one memory word.  No sum reaches 2^16, so adding the words adds the four fields.
template <int K> struct SgmRun;
template <> struct SgmRun<1> { using T = uint16_t; };
template <> struct SgmRun<2> { using T = uint32_t; };
template <> struct SgmRun<4> { using T = uint64_t; };

template <int K>
struct SgmStage {   // what a step loads
    uint64_t cl, cr[K];
    typename SgmRun<K>::T s;
};

template <int GROUP, int K>
__global__ __launch_bounds__(64 * SGM_WAVES) void sgm_path_kernel(const SgmArgs a, int dy, int dx, int first) {
    using Run = typename SgmRun<K>::T;
    const int t = threadIdx.x & 63;
    const int line = __builtin_amdgcn_readfirstlane((int)blockIdx.x * SGM_WAVES + ((int)threadIdx.x >> 6));
    int y, x, len;
    if (!sgm_line<GROUP>(a.xs0, a.xs1, a.ys0, a.ys1, line, dy, dx, y, x, len)) return;
    const int64_t HW = (int64_t)a.H * a.W;
    const uint64_t *cL = a.cen + (int64_t)blockIdx.y * HW, *cR = a.cen + ((int64_t)a.nc + blockIdx.y) * HW - a.dmin - K * t;
    uint16_t *S = a.S + sgm_s_offset(blockIdx.y, 0, 0, a.W, a.H, a.Dpad) + K * t;
    const bool in_run = K * t < a.Dpad;
    bool valid[K];
#pragma unroll
    for (int j = 0; j < K; ++j) valid[j] = K * t + j < a.D;
    const int64_t pix0 = (int64_t)y * a.W + x, step = (int64_t)dy * a.W + dx;
    auto load = [&](SgmStage<K> &st, int i) {
        const int64_t q = pix0 + i * step;
        st.cl = cL[q];
#pragma unroll
        for (int j = 0; j < K; ++j) st.cr[j] = valid[j] ? cR[q - j] : 0;   // x - d >= rw on a strict pixel
        st.s = !first && in_run ? *reinterpret_cast<const Run *>(S + q * a.Dpad) : (Run)0;
    };
    SgmStage<K> st[SGM_PREFETCH];
#pragma unroll
    for (int s = 0; s < SGM_PREFETCH; ++s)
        if (s < len) load(st[s], s);
    // L_r(p - r, .) and its minimum M; 0 in front of the first pixel makes the first step L = C by the same formula
    uint32_t Lp[K], M = 0u;
#pragma unroll
    for (int j = 0; j < K; ++j) Lp[j] = valid[j] ? 0u : SGM_BIG;
    for (int base = 0; base < len; base += SGM_PREFETCH) {
#pragma unroll
        for (int s = 0; s < SGM_PREFETCH; ++s) {   // unrolled: st[] is indexed by constants only
            const int i = base + s;
            if (i >= len) break;
            const SgmStage<K> cur = st[s];
            if (i + SGM_PREFETCH < len) load(st[s], i + SGM_PREFETCH);
            // the neighbours of the run's ends: lane t - 1's last and lane t + 1's first (BIG past either end of the wave)
            const uint32_t below = (uint32_t)__builtin_amdgcn_update_dpp((int)SGM_BIG, (int)Lp[K - 1], 0x138, 0xF, 0xF, false);   // wave_shr:1
            const uint32_t above = (uint32_t)__builtin_amdgcn_update_dpp((int)SGM_BIG, (int)Lp[0], 0x130, 0xF, 0xF, false);       // wave_shl:1
            const uint32_t jump = M + (uint32_t)a.p2;
            uint32_t Ln[K], m = SGM_BIG;
            Run add = 0;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const uint32_t lo = j > 0 ? Lp[j - 1] : below, hi = j < K - 1 ? Lp[j + 1] : above;
                const uint32_t best = min(min(Lp[j], jump), min(lo, hi) + (uint32_t)a.p1);
                Ln[j] = valid[j] ? sgm_cost(cur.cl, cur.cr[j]) + best - M : SGM_BIG;
                m = min(m, Ln[j]);
                add = (Run)(add | ((Run)(valid[j] ? Ln[j] : 0u) << (16 * j)));
            }
            if (in_run) *reinterpret_cast<Run *>(S + (pix0 + i * step) * a.Dpad) = (Run)(cur.s + add);
            M = stereo_wave_min(m);
#pragma unroll
            for (int j = 0; j < K; ++j) Lp[j] = Ln[j];
        }
    }
}

struct SgmSelectArgs {
    const uint16_t *S;
    int W, H, dmin, D, Dpad;
    int xs0, xs1, ys0, ys1;
    int64_t pair0;    // the first pair of this chunk: S is indexed by blockIdx.z, the planes below by pair0 + blockIdx.z
    int16_t *dR;      // (n, H, W)
    int uniq, lr, inv;
    const uint8_t *vL, *vR;
    int16_t *disp;
    int32_t *cost;     // or NULL
    uint8_t *status;   // or NULL
};

// d_R(y, x2) = the smallest d minimising S(y, x2 + d, d) over the d with (y, x2 + d) strict, for x2 in [xs0 - d_max, xs1 - 1 - d_min]:
// every x - d* of a strict pixel.  blockDim.x = SGM_RIGHT_TX.
__global__ __launch_bounds__(SGM_RIGHT_TX) void sgm_right_kernel(const SgmSelectArgs a) {
    __shared__ uint32_t rows[(SGM_RIGHT_TX + SGM_RIGHT_DC - 1) * SGM_RIGHT_ROW];
    const int t = threadIdx.x, y = a.ys0 + (int)blockIdx.y;
    const int x2_first = a.xs0 - (a.dmin + a.D - 1), x2_end = a.xs1 - a.dmin;   // exclusive
    const int x2_0 = x2_first + (int)blockIdx.x * SGM_RIGHT_TX, x2 = x2_0 + t;
    const uint16_t *Srow = a.S + sgm_s_offset(blockIdx.z, y, 0, a.W, a.H, a.Dpad);
    uint32_t best = STEREO_INF;
    int best_dl = 0;
    for (int c0 = 0; c0 < a.D; c0 += SGM_RIGHT_DC) {
        // row xi of the LDS: the disparities c0 .. c0 + DC - 1 of the left pixel x2_0 + dmin + c0 + xi
        const int xl0 = x2_0 + a.dmin + c0;
        for (int i = t; i < (SGM_RIGHT_TX + SGM_RIGHT_DC - 1) * (SGM_RIGHT_DC / 2); i += SGM_RIGHT_TX) {
            const int xi = i / (SGM_RIGHT_DC / 2), w = i % (SGM_RIGHT_DC / 2), xl = xl0 + xi;
            uint32_t v = 0u;
            if (xl >= a.xs0 && xl < a.xs1 && c0 + 2 * w < a.Dpad) v = *reinterpret_cast<const uint32_t *>(Srow + (int64_t)xl * a.Dpad + c0 + 2 * w);
            rows[xi * SGM_RIGHT_ROW + w] = v;
        }
        __syncthreads();
        for (int dd = 0; dd < SGM_RIGHT_DC; ++dd) {
            const int dl = c0 + dd, xl = x2 + a.dmin + dl;
            if (dl < a.D && xl >= a.xs0 && xl < a.xs1) {
                const uint32_t v = (rows[(t + dd) * SGM_RIGHT_ROW + dd / 2] >> (16 * (dd & 1))) & 0xFFFFu;
                if (v < best) best = v, best_dl = dl;   // ascending d: the smallest d of the smallest S
            }
        }
        __syncthreads();
    }
    if (x2 < x2_end) a.dR[((a.pair0 + blockIdx.z) * a.H + y) * a.W + x2] = (int16_t)(best == STEREO_INF ? STEREO_NO_DR : a.dmin + best_dl);
}

template <int K>
__global__ __launch_bounds__(64) void sgm_select_kernel(const SgmSelectArgs a) {
    using Run = typename SgmRun<K>::T;
    const int t = threadIdx.x, D = a.D;
    const int y = a.ys0 + (int)blockIdx.y, x0 = a.xs0 + 64 * (int)blockIdx.x, ncol = min(64, a.xs1 - x0);
    const uint16_t *Srow = a.S + sgm_s_offset(blockIdx.z, y, x0, a.W, a.H, a.Dpad);
    const bool in_run = K * t < a.Dpad;
    int my_dl = 0;
    uint32_t my_c = 0, my_c2 = STEREO_INF;
    for (int px = 0; px < ncol; ++px) {
        const Run run = in_run ? *reinterpret_cast<const Run *>(Srow + (int64_t)px * a.Dpad + K * t) : (Run)0;
        uint32_t v[K], best = STEREO_INF;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            v[j] = (uint32_t)(run >> (16 * j)) & 0xFFFFu;
            const int dl = K * t + j;
            best = min(best, dl < D ? (v[j] << 10) | (uint32_t)dl : STEREO_INF);
        }
        best = stereo_wave_min(best);
        const int dls = (int)(best & 1023u);
        uint32_t c2 = STEREO_INF;
        if (a.uniq > 0) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int dl = K * t + j;
                c2 = min(c2, dl < D && abs(dl - dls) >= 2 ? v[j] : STEREO_INF);
            }
            c2 = stereo_wave_min(c2);
        }
        if (t == px) my_dl = dls, my_c = best >> 10, my_c2 = c2;
    }
    if (t < ncol) {
        const int x = x0 + t, d = a.dmin + my_dl;
        const int64_t at = ((a.pair0 + blockIdx.z) * a.H + y) * a.W + x;
        int m = 0, p = 0;
        if (my_dl > 0 && my_dl < D - 1) {   // the winner's neighbours: this pixel's own run, just read
            const uint16_t *mine = Srow + (int64_t)t * a.Dpad + my_dl;
            m = mine[-1], p = mine[1];
        }
        int st = stereo_lookup_bits(d, at, a.lr, a.dR, a.vL, a.vR);
        if (stereo_not_unique(my_c2, my_c, a.uniq)) st |= STEREO_UNIQUENESS;
        a.disp[at] = (int16_t)(st ? a.inv : 16 * d + stereo_subpixel(my_dl, D, m, (int)my_c, p));
        if (a.cost) a.cost[at] = (int32_t)my_c;
        if (a.status) a.status[at] = (uint8_t)st;
    }
}

}  // namespace pcs
