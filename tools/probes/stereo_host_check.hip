// stereo_host_check.hip — stand-alone host check of csrc/pcs_stereo.inc for AddressSanitizer / UBSan; needs no device:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -o stereo_host_check stereo_host_check.hip && ./stereo_host_check
// It walks the argument checks of the three entry points (nothing there touches the device, and the handle is looked at last) and the
// tile / workspace arithmetic over the whole range of (num_disp, block): the tile fits the LDS budget, the kernel's LDS layout ends
// where the host says it does, and the strict rectangle, the strips and the grids cover the image without reaching outside it.
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
using namespace pcs;
template <int K> __global__ void membench_kernel(const double2 *, double2 *, int64_t) {}   // named by pcs_common.inc's pcs_membench
#include "../../pycamset_amd/csrc/pcs_common.inc"
#include "../../pycamset_amd/csrc/pcs_handle.inc"
#include "../../pycamset_amd/csrc/pcs_stereo.inc"

#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static bool names(const char *word) { return std::strstr(pcs_last_error(), word) != nullptr; }

int main() {
    const uint8_t *img = reinterpret_cast<const uint8_t *>(uintptr_t(64));   // never dereferenced on the host
    int16_t *disp = reinterpret_cast<int16_t *>(uintptr_t(64));
    auto match = [&](int W, int H, int64_t pl, int64_t pr, int mind, int D, int block, int cap, int tex, int uniq, int lr, const uint8_t *l = nullptr, const uint8_t *r = nullptr) {
        return pcs_stereo_match(nullptr, 1, W, H, l ? l : img, pl, r ? r : img, pr, mind, D, block, cap, tex, uniq, lr, nullptr, nullptr, disp, nullptr, nullptr, nullptr);
    };
    EXPECT(match(64, 32, 64, 64, 0, 16, 8, 31, 10, 15, -1) == PCS_ERR_ARG && names("block"));
    EXPECT(match(64, 32, 64, 64, 0, 16, 33, 31, 10, 15, -1) == PCS_ERR_ARG && names("block"));
    EXPECT(match(64, 32, 64, 64, 0, 0, 7, 31, 10, 15, -1) == PCS_ERR_ARG && names("num_disp"));
    EXPECT(match(64, 32, 64, 64, 0, 1025, 7, 31, 10, 15, -1) == PCS_ERR_ARG && names("num_disp"));
    EXPECT(match(64, 32, 64, 64, -1025, 16, 7, 31, 10, 15, -1) == PCS_ERR_ARG && names("min_disp"));
    EXPECT(match(64, 32, 64, 64, 0, 16, 7, 0, 10, 15, -1) == PCS_ERR_ARG && names("texture_threshold"));
    EXPECT(match(64, 32, 64, 64, 0, 16, 7, 64, 10, 15, -1) == PCS_ERR_ARG && names("prefilter_cap"));
    EXPECT(match(64, 32, 64, 64, 0, 16, 7, 31, 10, 101, -1) == PCS_ERR_ARG && names("uniqueness_ratio"));
    EXPECT(match(64, 32, 64, 64, 0, 16, 7, 31, 10, 15, -2) == PCS_ERR_ARG && names("lr_max_diff"));
    EXPECT(match(64, 32, 63, 64, 0, 16, 7, 31, 10, 15, -1) == PCS_ERR_ARG && names("left_pitch"));
    EXPECT(match(64, 32, 64, 8, 0, 16, 7, 31, 10, 15, -1) == PCS_ERR_ARG && names("right_pitch"));
    EXPECT(match(0, 32, 64, 64, 0, 16, 7, 31, 10, 15, -1) == PCS_ERR_ARG && names("width"));
    EXPECT(match(64, 70000, 64, 64, 0, 16, 7, 31, 10, 15, -1) == PCS_ERR_ARG && names("height"));
    EXPECT(pcs_stereo_match(nullptr, 1, 64, 32, nullptr, 64, img, 64, 0, 16, 7, 31, 10, 15, -1, nullptr, nullptr, disp, nullptr, nullptr, nullptr) == PCS_ERR_ARG && names("d_left"));
    EXPECT(pcs_stereo_match(nullptr, 1, 64, 32, img, 64, img, 64, 0, 16, 7, 31, 10, 15, -1, img, nullptr, disp, nullptr, nullptr, nullptr) == PCS_ERR_ARG && names("d_valid_left"));
    EXPECT(pcs_stereo_match(nullptr, 1, 64, 32, img, 64, img, 64, 0, 16, 7, 31, 10, 15, -1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == PCS_ERR_ARG && names("d_disp"));
    EXPECT(match(64, 32, 64, 64, 0, 16, 7, 31, 10, 15, -1) == PCS_ERR_ARG && names("handle"));   // everything else was in order

    double Q[32] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    void *buf = reinterpret_cast<void *>(uintptr_t(64));
    uint8_t *mask = reinterpret_cast<uint8_t *>(uintptr_t(64));
    EXPECT(pcs_stereo_reproject(nullptr, 1, 8, 8, disp, 0, nullptr, 1, 0, 1, nullptr, buf, PCS_F32, mask, nullptr, nullptr) == PCS_ERR_ARG && names("Q"));
    EXPECT(pcs_stereo_reproject(nullptr, 2, 8, 8, disp, 0, Q, 3, 0, 1, nullptr, buf, PCS_F32, mask, nullptr, nullptr) == PCS_ERR_ARG && names("n_Q"));
    Q[5] = NAN;
    EXPECT(pcs_stereo_reproject(nullptr, 1, 8, 8, disp, 0, Q, 1, 0, 1, nullptr, buf, PCS_F32, mask, nullptr, nullptr) == PCS_ERR_ARG && names("Q of pair 0"));
    Q[5] = 1, T[11] = INFINITY;
    EXPECT(pcs_stereo_reproject(nullptr, 1, 8, 8, disp, 0, Q, 1, 0, 1, T, buf, PCS_F32, mask, nullptr, nullptr) == PCS_ERR_ARG && names("T"));
    EXPECT(pcs_stereo_reproject(nullptr, 1, 8, 8, disp, 0, Q, 1, NAN, 1, nullptr, buf, PCS_F32, mask, nullptr, nullptr) == PCS_ERR_ARG && names("z_lo"));
    EXPECT(pcs_stereo_reproject(nullptr, 1, 8, 8, disp, 0, Q, 1, 0, 1, nullptr, buf, PCS_MIXED, mask, nullptr, nullptr) == PCS_ERR_ARG && names("dtype"));
    EXPECT(pcs_stereo_reproject(nullptr, 1, 8, 8, disp, 0, Q, 1, 0, 1, nullptr, buf, PCS_F64, nullptr, nullptr, nullptr) == PCS_ERR_ARG && names("d_mask"));
    EXPECT(pcs_stereo_reproject(nullptr, 1, 8, 8, disp, 0, Q, 1, 0, 1, nullptr, buf, PCS_F64, mask, nullptr, nullptr) == PCS_ERR_ARG && names("handle"));
    int64_t *counts = reinterpret_cast<int64_t *>(uintptr_t(64));
    EXPECT(pcs_stereo_compact(nullptr, 1, 8, 8, buf, PCS_F32, mask, mask, 7, buf, mask, counts, nullptr) == PCS_ERR_ARG && names("values_pitch"));
    EXPECT(pcs_stereo_compact(nullptr, 1, 8, 8, buf, PCS_F32, mask, mask, 8, buf, nullptr, counts, nullptr) == PCS_ERR_ARG && names("d_out_values"));
    EXPECT(pcs_stereo_compact(nullptr, 1, 8, 8, buf, PCS_F32, mask, nullptr, 0, buf, nullptr, nullptr, nullptr) == PCS_ERR_ARG && names("d_counts"));
    EXPECT(pcs_stereo_compact(nullptr, 40000, 8, 8, buf, PCS_F32, mask, nullptr, 0, buf, nullptr, counts, nullptr) == PCS_ERR_ARG && names("n 40000"));
    EXPECT(pcs_stereo_compact(nullptr, 1, 8, 8, buf, PCS_F32, mask, nullptr, 0, buf, nullptr, counts, nullptr) == PCS_ERR_ARG && names("handle"));
    EXPECT(pcs_stereo_destroy(nullptr) == PCS_OK);

    // the tiling over every (num_disp, block), a few shapes and ranges
    long tiles = 0;
    for (int D = 1; D <= STEREO_MAX_DISP; D += (D < 70 ? 1 : 37))
        for (int block = 3; block <= STEREO_MAX_BLOCK; block += 2)
            for (int mind : {-1024, -7, 0, 3, 1024})
                for (int W : {1, 31, 64, 65, 2448, 65535})
                    for (int H : {1, block, block + 1, 33, 2048})
                        for (int64_t n : {int64_t(1), int64_t(16)}) {
                            const StereoTiling t = stereo_tiling(n, W, H, mind, D, block);
                            ++tiles;
                            EXPECT(t.r == block / 2 && t.Dpad >= D && t.Dpad == 64 * t.K && t.K <= STEREO_MAX_K && (t.K == 1 || 32 * t.K < D));
                            EXPECT(t.TW >= 1 && t.TW <= STEREO_MAX_TW && t.lds == stereo_lds_bytes(t.TW, t.r, t.Dpad) && t.lds <= STEREO_LDS_LIMIT);
                            for (int want : {1, 7, 64, 1000}) {   // an override is honoured where it fits and narrowed where it does not
                                const StereoTiling o = stereo_tiling(n, W, H, mind, D, block, want, 3);
                                EXPECT(o.TW >= 1 && o.TW <= std::min(want, STEREO_MAX_TW) && o.lds <= STEREO_LDS_LIMIT && o.SH == 3);
                                EXPECT(o.TW == std::min(want, STEREO_MAX_TW) || stereo_lds_bytes(o.TW + 1, o.r, o.Dpad) > STEREO_LDS_LIMIT);
                            }
                            // the kernel's layout: column sums, texture sums, two anchor rows, two other rows — the last byte is the host's
                            const int TWH = t.TW + 2 * t.r, TWHp = stereo_pad4(TWH), SEGp = stereo_pad4(TWH + t.Dpad - 1);
                            EXPECT((int64_t)2 * TWH * t.Dpad + 2 * TWHp + 2 * TWHp + 2 * SEGp == t.lds && (2 * TWH * t.Dpad + 2 * TWHp) % 4 == 0);
                            EXPECT(t.SH >= STEREO_MIN_STRIP && t.SH <= 256);
                            EXPECT(t.xs0 <= t.xs1 && t.ys0 <= t.ys1 && t.xr0 <= t.xr1);
                            if (t.xs1 > t.xs0 && t.ys1 > t.ys0) {
                                // every window of a strict pixel, in both images and for both ends of the range, lies inside the image
                                const int dmax = mind + D - 1;
                                EXPECT(t.xs0 - t.r >= 0 && t.xs1 - 1 + t.r <= W - 1 && t.ys0 - t.r >= 0 && t.ys1 - 1 + t.r <= H - 1);
                                EXPECT(t.xs0 - dmax - t.r >= 0 && t.xs1 - 1 - mind + t.r <= W - 1);
                                EXPECT(t.xr0 <= t.xs0 - dmax && t.xs1 - 1 - mind < t.xr1);   // x - d* is a pixel the right-anchored pass wrote
                                const int gx = (t.xs1 - t.xs0 + t.TW - 1) / t.TW, gy = (t.ys1 - t.ys0 + t.SH - 1) / t.SH;
                                EXPECT(gx >= 1 && gy >= 1 && (gx - 1) * t.TW < t.xs1 - t.xs0 && (gy - 1) * t.SH < t.ys1 - t.ys0 && gy <= 65535);
                            }
                            EXPECT(stereo_match_workspace(n, W, H) == n * (int64_t)W * H * 4);
                            EXPECT(stereo_blocks_per_pair(W, H) * STEREO_PIX_PER_BLOCK >= (int64_t)W * H && (stereo_blocks_per_pair(W, H) - 1) * STEREO_PIX_PER_BLOCK < (int64_t)W * H);
                        }
    std::printf("stereo_host_check ok (%ld tilings)\n", tiles);
    return 0;
}
