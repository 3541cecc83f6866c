// sgm_host_check.hip — stand-alone host check of the semi-global part of csrc/pcs_stereo.inc for AddressSanitizer / UBSan; needs no device:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -o sgm_host_check sgm_host_check.hip && ./sgm_host_check
// It walks the argument checks of pcs_stereo_sgm and pcs_stereo_set_sgm_workspace (nothing there touches the device, and the handle is
// looked at last), the sizing functions the host shares with the kernels (sgm_k, sgm_dpad, sgm_s_offset, sgm_pair_bytes, the chunk
// size under a limit), and the line geometry of the path kernel: for every direction the lines of sgm_line visit every pixel of the
// strict rectangle exactly once, start where p - r is outside it and never leave it; a lane's run of S stays inside its pixel's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/pcs_hip.h"
#include "../../pycamset_amd/csrc/ba_device.hpp"
#include "../../pycamset_amd/csrc/ba_prior.hpp"
#include "../../pycamset_amd/csrc/ba_bounds.hpp"
#include "../../pycamset_amd/csrc/ba_triangulate.hpp"
#include "../../pycamset_amd/csrc/ba_stereo.hpp"
#include "../../pycamset_amd/csrc/ba_stereo_sgm.hpp"
using namespace pcs;
template <int K> __global__ void membench_kernel(const double2 *, double2 *, int64_t) {}   // named by pcs_common.inc's pcs_membench
#include "../../pycamset_amd/csrc/pcs_common.inc"
#include "../../pycamset_amd/csrc/pcs_handle.inc"
#include "../../pycamset_amd/csrc/pcs_stereo.inc"

#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool names(const char *word) { return std::strstr(pcs_last_error(), word) != nullptr; }

template <int GROUP>
static bool lines_cover(int xs0, int xs1, int ys0, int ys1, int dy, int dx) {
    const int Ws = xs1 - xs0, Hs = ys1 - ys0, n = sgm_line_count(GROUP, Ws, Hs);
    std::vector<int> seen((size_t)Ws * Hs, 0);
    auto inside = [&](int y, int x) { return y >= ys0 && y < ys1 && x >= xs0 && x < xs1; };
    int y = 0, x = 0, len = 0;
    for (int line = 0; line < n; ++line) {
        if (!sgm_line<GROUP>(xs0, xs1, ys0, ys1, line, dy, dx, y, x, len) || len < 1) return false;
        if (!inside(y, x) || inside(y - dy, x - dx)) return false;                              // a path starts where p - r is not strict
        if (!inside(y + (len - 1) * dy, x + (len - 1) * dx) || inside(y + len * dy, x + len * dx)) return false;   // and runs to the other edge
        for (int i = 0; i < len; ++i) ++seen[(size_t)(y + i * dy - ys0) * Ws + (x + i * dx - xs0)];
    }
    if (sgm_line<GROUP>(xs0, xs1, ys0, ys1, n, dy, dx, y, x, len)) return false;   // the waves past the last line of a grid do nothing
    return std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; });
}

int main() {
    const uint8_t *img = reinterpret_cast<const uint8_t *>(uintptr_t(64));   // never dereferenced on the host
    int16_t *disp = reinterpret_cast<int16_t *>(uintptr_t(64));
    auto sgm = [&](int W, int H, int64_t pl, int64_t pr, int mind, int D, int cw, int ch, int p1, int p2, int paths, int uniq, int lr) {
        return pcs_stereo_sgm(nullptr, 1, W, H, img, pl, img, pr, mind, D, cw, ch, p1, p2, paths, uniq, lr, nullptr, nullptr, disp, nullptr, nullptr, nullptr);
    };
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 4, 7, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("census_w"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 1, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("census_h"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 9, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("80 bits"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 65535, 65535, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("bits"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 7, 33, 32, 8, 15, -1) == PCS_ERR_ARG && names("p1"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 7, -1, 32, 8, 15, -1) == PCS_ERR_ARG && names("p1"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 7, 8, 1024, 8, 15, -1) == PCS_ERR_ARG && names("p2"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 7, 8, 32, 6, 15, -1) == PCS_ERR_ARG && names("paths"));
    EXPECT(sgm(64, 32, 64, 64, 0, 0, 9, 7, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("num_disp"));
    EXPECT(sgm(64, 32, 64, 64, 0, 257, 9, 7, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("num_disp"));
    EXPECT(sgm(64, 32, 64, 64, 1025, 16, 9, 7, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("min_disp"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 7, 8, 32, 8, 101, -1) == PCS_ERR_ARG && names("uniqueness_ratio"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 7, 8, 32, 8, 15, -2) == PCS_ERR_ARG && names("lr_max_diff"));
    EXPECT(sgm(64, 32, 63, 64, 0, 16, 9, 7, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("left_pitch"));
    EXPECT(sgm(64, 32, 64, 8, 0, 16, 9, 7, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("right_pitch"));
    EXPECT(sgm(0, 32, 64, 64, 0, 16, 9, 7, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("width"));
    EXPECT(pcs_stereo_sgm(nullptr, 1, 64, 32, nullptr, 64, img, 64, 0, 16, 9, 7, 8, 32, 8, 15, -1, nullptr, nullptr, disp, nullptr, nullptr, nullptr) == PCS_ERR_ARG && names("d_left"));
    EXPECT(pcs_stereo_sgm(nullptr, 1, 64, 32, img, 64, img, 64, 0, 16, 9, 7, 8, 32, 8, 15, -1, img, nullptr, disp, nullptr, nullptr, nullptr) == PCS_ERR_ARG && names("d_valid_left"));
    EXPECT(pcs_stereo_sgm(nullptr, 1, 64, 32, img, 64, img, 64, 0, 16, 9, 7, 8, 32, 8, 15, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PCS_ERR_ARG && names("d_disp"));
    EXPECT(sgm(64, 32, 64, 64, 0, 16, 9, 7, 8, 32, 8, 15, -1) == PCS_ERR_ARG && names("handle"));             // everything else was in order
    EXPECT(sgm(64, 32, 64, 64, -1024, 256, 13, 5, 0, 1023, 4, 100, 0) == PCS_ERR_ARG && names("handle"));     // the limits themselves
    EXPECT(pcs_stereo_set_sgm_workspace(nullptr, -1) == PCS_ERR_ARG && names("bytes"));
    EXPECT(pcs_stereo_set_sgm_workspace(nullptr, 0) == PCS_ERR_ARG && names("handle"));

    // sizing: shared by host and kernels
    long shapes = 0;
    for (int D = 1; D <= SGM_MAX_DISP; ++D) {
        const int K = sgm_k(D), Dpad = sgm_dpad(D);
        EXPECT((K == 1 || K == 2 || K == 4) && 64 * K >= D && Dpad >= D && Dpad < D + 4 && Dpad % 4 == 0 && Dpad % K == 0);
        EXPECT(8 * (SGM_MAX_BITS + SGM_MAX_P) < (1 << 14) && SGM_MAX_DISP <= 1024 && SGM_BIG + SGM_MAX_P > SGM_BIG);   // S << 10 | k fits the wave-minimum key
        for (int t = 0; t < 64; ++t)   // a lane's run lies inside its pixel's Dpad elements or the lane stays out, and covers every disparity
            EXPECT(K * t >= Dpad || K * t + K <= Dpad);
        EXPECT(K * 63 + K >= D);
        for (int W : {1, 31, 64, 2448, 65535})
            for (int H : {1, 7, 33, 2048, 65535}) {
                ++shapes;
                const int64_t per = sgm_pair_bytes(W, H, Dpad);
                EXPECT(per == (int64_t)2 * H * W * Dpad + (int64_t)16 * H * W && per > 0);
                EXPECT(sgm_s_offset(3, H - 1, W - 1, W, H, Dpad) + Dpad == sgm_s_offset(4, 0, 0, W, H, Dpad));   // the last run of a pair ends where the next pair begins
                EXPECT((2 * sgm_s_offset(5, 0, 0, W, H, Dpad)) % 8 == 0);                                         // the census planes behind S are 8-byte aligned
                EXPECT(sgm_chunk_pairs(16, per, per - 1) == 0 && sgm_chunk_pairs(16, per, per) == 1 && sgm_chunk_pairs(16, per, 3 * per + per / 2) == 3);
                EXPECT(sgm_chunk_pairs(2, per, 100 * per) == 2 && sgm_chunk_pairs(5, per, 0) == std::min<int64_t>(5, SGM_DEFAULT_WORKSPACE / per));
            }
    }
    // the strict rectangle and the lines of every direction over it
    long rects = 0;
    static const int dirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
    for (int D : {1, 16, 65, 256})
        for (int mind : {-1024, -7, 0, 3, 128})
            for (int cw : {3, 9, 13})
                for (int ch : {3, 5})
                    for (int W : {1, cw, cw + D - 1, cw + D, cw + D + 5, cw + D + 40})
                        for (int H : {1, ch - 1, ch, ch + 1, ch + 9, ch + 70}) {
                            const SgmPlan t = sgm_plan(W, H, mind, D, cw, ch);
                            const int dmax = mind + D - 1;
                            EXPECT(t.xs0 <= t.xs1 && t.ys0 <= t.ys1 && t.K == sgm_k(D) && t.Dpad == sgm_dpad(D) && t.pair_bytes == sgm_pair_bytes(W, H, t.Dpad));
                            if (t.xs1 == t.xs0 || t.ys1 == t.ys0) continue;
                            ++rects;
                            // both census windows of a strict pixel, for both ends of the range, lie inside the image
                            EXPECT(t.xs0 - t.rw >= 0 && t.xs1 - 1 + t.rw <= W - 1 && t.ys0 - t.rh >= 0 && t.ys1 - 1 + t.rh <= H - 1);
                            EXPECT(t.xs0 - dmax - t.rw >= 0 && t.xs1 - 1 - mind + t.rw <= W - 1);
                            // the right-anchored pass writes every x - d* the selection reads, inside the image
                            const int Ws = t.xs1 - t.xs0, x2_first = t.xs0 - dmax, x2_end = t.xs1 - mind;
                            EXPECT(x2_first >= 0 && x2_end <= W && x2_end - x2_first == Ws + D - 1);
                            for (int i = 0; i < 8; ++i) {
                                const int dy = dirs[i][0], dx = dirs[i][1];
                                const bool ok = dy == 0 ? lines_cover<SGM_HORIZONTAL>(t.xs0, t.xs1, t.ys0, t.ys1, dy, dx)
                                              : dx == 0 ? lines_cover<SGM_VERTICAL>(t.xs0, t.xs1, t.ys0, t.ys1, dy, dx)
                                                        : lines_cover<SGM_DIAGONAL>(t.xs0, t.xs1, t.ys0, t.ys1, dy, dx);
                                EXPECT(ok);
                            }
                        }
    std::printf("sgm_host_check ok (%ld shapes, %ld strict rectangles)\n", shapes, rects);
    return 0;
}
