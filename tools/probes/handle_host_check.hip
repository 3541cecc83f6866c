// handle_host_check.hip — stand-alone host check of csrc/pcs_handle.inc for AddressSanitizer / UBSan; needs no device:
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined -o handle_host_check handle_host_check.hip && ./handle_host_check
// Without a device every hipMalloc fails, so this walks the slot table's host logic and the error paths of DevBuf (a failed grow leaves an
// empty buffer, release of an empty buffer is a no-op); with a device it also grows, substitutes and releases.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>

#include "../../include/pcs_hip.h"
#include "../../pycamset_amd/csrc/ba_triangulate.hpp"
using namespace pcs;
template <int K> __global__ void membench_kernel(const double2 *, double2 *, int64_t) {}   // named by pcs_common.inc's pcs_membench
#include "../../pycamset_amd/csrc/pcs_common.inc"
#include "../../pycamset_amd/csrc/pcs_handle.inc"

#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    const bool dev = pcs_device_count() > 0;
    DevBuf a, b, c;
    double caller[4] = {};
    OutSlot sl[3] = {{1, a, nullptr, 8, sizeof(double)}, {2, b, caller, 8, sizeof(double)}, {4, c, nullptr, 0, sizeof(double)}};
    bool grows = false;
    EXPECT(owned_slots(sl + 1, 2, &grows) == 4 && !grows);   // the caller's slot is not owned; an empty owned slot frees nothing: no wait
    EXPECT(owned_slots(sl, 3, &grows) == 5 && grows);
    EXPECT(check_lm_options("t", 1, 0.0, 0.0, 0.0, false, "x") == PCS_ERR_ARG);
    EXPECT(check_lm_options("t", 1, 0.0, 0.0, 0.0, true, "x") == PCS_OK && check_lm_options("t", -1, 0.0, 0.0, 0.0, true, "x") == PCS_ERR_ARG);
    EXPECT(check_lm_options("t", 1, NAN, 0.0, 0.0, true, "x") == PCS_ERR_ARG && check_lm_options("t", 1, 0.0, INFINITY, 0.0, true, "x") == PCS_ERR_ARG);
    const int rc = grow_owned_slots(sl, 3);
    if (dev) {
        EXPECT(rc == PCS_OK && sl[0].ptr == a.p && a.cap == 8 && sl[1].ptr == caller && !b.p && sl[2].ptr == c.p && c.cap == 1);
        void *old = a.p;
        EXPECT(a.grow(4, sizeof(double)) == PCS_OK && a.p == old && a.cap == 8);   // no shrink, no reallocation
    } else {
        EXPECT(rc == PCS_ERR_HIP && !a.p && a.cap == 0 && !sl[0].ptr && sl[1].ptr == caller);   // nothing substituted by the failed call
        EXPECT(open_device("t", 0) == PCS_ERR_NODEVICE);
    }
    RunFence f;   // never recorded: nothing to wait for, whatever the stream
    EXPECT(f.wait_host() == hipSuccess && f.before_run(nullptr, true) == hipSuccess);
    KernelTimer t;
    float ms = 0;
    EXPECT(timer_ms("t", nullptr, &ms, "x") == PCS_ERR_ARG && timer_ms("t", &t, &ms, "nothing has run yet") == PCS_ERR_STATE);
    const OutSlot want[2] = {{1, a, nullptr, 8, sizeof(double)}, {2, b, caller, 8, sizeof(double)}};
    HandleCore core;
    EXPECT(fetch_slots(core, want, 2, 1, false, "t", "refused") == PCS_ERR_STATE);   // slot 2 was the caller's: refused before any device call
    EXPECT(fetch_slots(core, want, 1, 1, false, "t", "refused") == PCS_OK);
    for (DevBuf *d : {&a, &b, &c}) d->release();
    t.destroy();
    f.destroy();
    std::printf("handle_host_check ok (%s)\n", dev ? "with a device" : "no device: error paths");
    return 0;
}
