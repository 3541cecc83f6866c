// dettable_host_check.hip — stand-alone host check of csrc/pcs_dettable.inc and of the set_observations checker of csrc/pcs_handle.inc for
// AddressSanitizer / UBSan; needs no device:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -o dettable_host_check dettable_host_check.hip && ./dettable_host_check
// Parsing, the range check, the width rule and the packing are host-only.  Without a device every hipMalloc fails, so the upload is
// walked as the failure it then is (no detections set, empty buffers); with a device it also succeeds once in each form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/pcs_hip.h"
#include "../../pycamset_amd/csrc/ba_device.hpp"
#include "../../pycamset_amd/csrc/ba_triangulate.hpp"
using namespace pcs;
template <int K> __global__ void membench_kernel(const double2 *, double2 *, int64_t) {}   // named by pcs_common.inc's pcs_membench
#include "../../pycamset_amd/csrc/pcs_common.inc"
#include "../../pycamset_amd/csrc/pcs_handle.inc"
#include "../../pycamset_amd/csrc/pcs_dettable.inc"

#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, pcs_last_error()); return 1; } } while (0)
static bool said(const char *text) { return std::strstr(pcs_last_error(), text) != nullptr; }

// the decoding of csrc/ba_device.hpp, restated
static void decode(uint32_t w, const DetWidths &b, int32_t *cam, int32_t *img, int32_t *key) {
    *key = (int32_t)(w & (((uint64_t)1 << b.key_bits) - 1));
    *img = (int32_t)((w >> b.key_bits) & (((uint64_t)1 << b.img_bits) - 1));
    *cam = (int32_t)((uint64_t)w >> (b.key_bits + b.img_bits));
}

int main() {
    const bool dev = pcs_device_count() > 0;
    DetColumns c;
    std::vector<double> uv;

    // ---- parse: what is not an index is refused, the first bad entry by row, then by column
    const double good[10] = {2, 3, 19, 0.5, 1.5, 0.9, 0, 7, -2.5, 1e9};   // 0.9 truncates to 0 like int()
    EXPECT(det_parse(good, 2, c, uv) == PCS_OK && c.cam == std::vector<int32_t>({2, 0}) && c.img == std::vector<int32_t>({3, 0}) &&
           c.key == std::vector<int32_t>({19, 7}) && uv == std::vector<double>({0.5, 1.5, -2.5, 1e9}));
    EXPECT(det_parse(good, 0, c, uv) == PCS_OK && c.cam.empty() && uv.empty());
    for (const double bad : {(double)NAN, -1.0, 2147483648.0, (double)INFINITY})
        for (int col = 0; col < 3; ++col) {
            double t[10];
            std::memcpy(t, good, sizeof(t));
            t[5 + col] = bad;
            char want[64];
            std::snprintf(want, sizeof(want), "detection 1: index column %d = ", col);
            EXPECT(det_parse(t, 2, c, uv) == PCS_ERR_RANGE && said(want) && said("is not an index"));
        }
    {
        double t[10];
        std::memcpy(t, good, sizeof(t));
        t[1] = 2147483647.0, t[2] = -0.5;   // the largest index; -0.5 truncates to 0
        EXPECT(det_parse(t, 2, c, uv) == PCS_OK && c.img[0] == INT32_MAX && c.key[0] == 0);
        t[7] = NAN, t[0] = 5;   // row 0 out of range AND row 1 not an index
        const DetCounts m{3, INT32_MAX, 20, false};
        EXPECT(det_parse(t, 2, c, uv, &m) == PCS_ERR_RANGE && said("detection 0 = (cam 5,"));   // checked row by row: the first bad row wins
        EXPECT(det_parse(t, 2, c, uv) == PCS_ERR_RANGE && said("detection 1: index column 2"));   // parse only
    }

    // ---- range check, per column; the table without an image column
    const DetCounts rig{3, 4, 20, false}, free_chain{3, 0, 20, true};
    auto cols = [](int32_t cam, int32_t img, int32_t key) {
        DetColumns d;
        d.cam = {0, cam}, d.img = {0, img}, d.key = {0, key};
        return d;
    };
    EXPECT(det_check_range(cols(2, 3, 19), rig) == PCS_OK);
    EXPECT(det_check_range(cols(3, 3, 19), rig) == PCS_ERR_RANGE && said("detection 1 = (cam 3, im 3, key 19) outside (3, 4, 20)"));
    EXPECT(det_check_range(cols(2, 4, 19), rig) == PCS_ERR_RANGE && det_check_range(cols(2, 3, 20), rig) == PCS_ERR_RANGE);
    EXPECT(det_check_range(cols(-1, 3, 19), rig) == PCS_ERR_RANGE && det_check_range(cols(2, -1, 19), rig) == PCS_ERR_RANGE &&
           det_check_range(cols(2, 3, -1), rig) == PCS_ERR_RANGE);
    EXPECT(det_check_range(cols(2, 12345, 19), free_chain) == PCS_OK && det_check_range(cols(2, -7, 19), free_chain) == PCS_OK);   // image values unchecked
    EXPECT(det_check_range(cols(3, 0, 19), free_chain) == PCS_ERR_RANGE && det_check_range(cols(2, 0, 20), free_chain) == PCS_ERR_RANGE);

    // ---- the width rule at its edge
    auto widths = [](int64_t cams, int64_t imgs, int64_t keys, bool no_img = false) { return det_widths(DetCounts{cams, imgs, keys, no_img}); };
    EXPECT(det_bits_for(1) == 0 && det_bits_for(2) == 1 && det_bits_for(3) == 2 && det_bits_for(4) == 2 && det_bits_for(5) == 3);
    EXPECT(widths(1 << 10, 1 << 10, 1 << 12).packs);             // 10 + 10 + 12 = 32
    EXPECT(!widths((1 << 10) + 1, 1 << 10, 1 << 12).packs);      // 11 + 10 + 12 = 33
    EXPECT(!widths(513, 513, 4097).packs);                       // 10 + 10 + 13 = 33
    EXPECT(widths(2, 1 << 15, 1 << 16).packs);                   // 1 + (15 + 16 = 31)
    EXPECT(!widths(1, 1 << 16, 1 << 16).packs);                  // 0 + 32 bits: key_bits + img_bits == 32 does not pack (the shift of the camera field)
    const DetWidths fw = widths(1 << 6, 1 << 20, 1 << 26, true);
    EXPECT(fw.img_bits == 0 && fw.key_bits == 26 && fw.packs);   // no image column: it takes no bits

    // ---- every packed word decodes to its triple (fields at their largest values, at the 32-bit edge)
    {
        const DetCounts m{1 << 10, 1 << 10, 1 << 12, false};
        const DetWidths w = det_widths(m);
        DetColumns d;
        for (int32_t cam : {0, 1, 511, 1023})
            for (int32_t img : {0, 1, 512, 1023})
                for (int32_t key : {0, 1, 2048, 4095}) d.cam.push_back(cam), d.img.push_back(img), d.key.push_back(key);
        EXPECT(det_check_range(d, m) == PCS_OK);
        const std::vector<uint32_t> word = det_pack(d, w);
        EXPECT(word.size() == d.cam.size() && word.back() == 0xffffffffu);
        for (size_t i = 0; i < word.size(); ++i) {
            int32_t cam, img, key;
            decode(word[i], w, &cam, &img, &key);
            EXPECT(cam == d.cam[i] && img == d.img[i] && key == d.key[i]);
        }
        DetColumns f = d;
        for (int32_t &v : f.img) v = 999;   // no image column: whatever it holds stays out of the word
        const std::vector<uint32_t> fword = det_pack(f, fw);
        for (size_t i = 0; i < fword.size(); ++i) EXPECT(fword[i] == (((uint32_t)f.cam[i] << 26) | (uint32_t)f.key[i]));
    }

    // ---- the set_observations checker: each refusal, and which one wins
    {
        const char *who = "t";
        const int32_t key[4] = {0, 1, 2, 3};
        const int64_t start[4] = {0, 2, 2, 4};
        int visited = 0;
        auto all_ok = [&](int64_t) { ++visited; return (int)PCS_OK; };
        EXPECT(check_grouped_observations(who, 4, key, 4, 3, start, all_ok) == PCS_OK && visited == 3);   // an empty group is fine
        const int64_t none[1] = {0};
        EXPECT(check_grouped_observations(who, 0, nullptr, 4, 0, none, all_ok) == PCS_OK);
        const int64_t late[4] = {1, 2, 2, 4}, shorter[4] = {0, 2, 2, 3}, back[4] = {0, 3, 2, 4};
        EXPECT(check_grouped_observations(who, 4, key, 4, 3, late, all_ok) == PCS_ERR_ARG && said("t: start_inds must run from 0 to n_obs"));
        EXPECT(check_grouped_observations(who, 4, key, 4, 3, shorter, all_ok) == PCS_ERR_ARG && said("must run from 0 to n_obs"));
        EXPECT(check_grouped_observations(who, 4, key, 4, 3, back, all_ok) == PCS_ERR_ARG && said("t: start_inds must be non-decreasing"));
        EXPECT(check_grouped_observations(who, 4, key, 3, 3, start, all_ok) == PCS_ERR_RANGE && said("observation 3 has key 3 outside [0,3)"));
        const int32_t neg[4] = {0, -1, 2, 3};
        EXPECT(check_grouped_observations(who, 4, neg, 4, 3, start, all_ok) == PCS_ERR_RANGE && said("observation 1 has key -1 outside [0,4)"));
        // several at once: the ends of start_inds first; then group by group, a group's start index before its own columns; indices last
        const int32_t cam_of[3] = {0, 9, 0};
        auto group_ok = [&](int64_t j) { return check_group_entity("view", j, "camera", cam_of[j], 2); };
        const int64_t back_late[4] = {1, 3, 2, 4}, back_at_2[4] = {0, 2, 5, 4}, back_at_1[4] = {0, 5, 2, 4};
        EXPECT(check_grouped_observations(who, 4, neg, 3, 3, back_late, group_ok) == PCS_ERR_ARG && said("must run from 0 to n_obs"));
        EXPECT(check_grouped_observations(who, 4, neg, 3, 3, back_at_2, group_ok) == PCS_ERR_RANGE && said("view 1 has camera 9 outside [0,2)"));   // group 1's column before group 2's start
        EXPECT(check_grouped_observations(who, 4, neg, 3, 3, back_at_1, group_ok) == PCS_ERR_ARG && said("non-decreasing"));   // group 1's start before group 1's column
        EXPECT(check_grouped_observations(who, 4, neg, 3, 3, start, group_ok) == PCS_ERR_RANGE && said("view 1 has camera"));   // a bad group before a bad index
        EXPECT(check_group_entity("group", 7, "image", 4, 4) == PCS_ERR_RANGE && said("group 7 has image 4 outside [0,4)") && check_group_entity("group", 7, "image", 3, 4) == PCS_OK);
    }

    // ---- upload: n is set last, so a failure leaves "no detections set" and, when it is the first allocation that fails, empty buffers
    {
        DetStore st;
        const double uvs[4] = {1.25, 2.5, 3.75, 5.0};
        for (const bool pack : {true, false})
            for (const bool f32 : {false, true}) {
                DetColumns d = cols(2, 3, 19);
                const int rc = st.upload(d, uvs, rig, pack, f32);
                EXPECT(d.cam.empty());   // taken over either way
                if (dev) {
                    EXPECT(rc == PCS_OK && st.n == 2 && st.uv_f32 == f32 && st.key_bits == 5 && st.img_bits == 2 && st.h.key == std::vector<int32_t>({0, 19}));
                    EXPECT(pack ? (st.packed.p && !st.cam.p && !st.img.p && !st.key.p) : (!st.packed.p && st.cam.p && st.img.p && st.key.p));
                    const DetTable t = st.table();
                    EXPECT(t.packed == st.packed.p && t.cam == st.cam.p && t.uv == st.uv.p && t.key_bits == 5 && t.img_bits == 2 && (t.uv_f32 != 0) == f32);
                } else {
                    EXPECT(rc == PCS_ERR_HIP && st.n == 0);
                    for (const DevBuf *b : {&st.packed, &st.cam, &st.img, &st.key, &st.uv}) EXPECT(!b->p && b->cap == 0);
                    EXPECT(!st.table().packed && !st.table().cam && !st.table().uv);
                }
            }
        DetColumns nothing;
        EXPECT(st.upload(nothing, nullptr, rig, true, false) == PCS_OK && st.n == 0 && !st.packed.p && !st.uv.p && st.h.cam.empty());   // an empty table needs no device
        st.release();
        st.release();   // of an empty store: a no-op
    }
    std::printf("dettable_host_check ok (%s)\n", dev ? "with a device" : "no device: error paths");
    return 0;
}
