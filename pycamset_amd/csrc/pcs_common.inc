// pcs_common.inc — what every part of the host side shares (included first by pcs_engine.hip): the error text, HIPCHK, the device
// queries and the handle-free utilities of the C ABI.

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return fail(PCS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

static int device_cu_count(int device) {
    static std::atomic<int> cached[64];
    if (device < 0 || device >= 64) return 0;
    int v = cached[device].load();
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) v = 0;
        cached[device].store(v);
    }
    return v;
}

extern "C" {
int pcs_version(void) { return 130; }
const char *pcs_last_error(void) { return g_err.c_str(); }

int pcs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pcs_host_alloc(void **out, int64_t bytes) {
    if (!out || bytes <= 0) return fail(PCS_ERR_ARG, "pcs_host_alloc: bad arguments");
    *out = nullptr;
    HIPCHK(hipHostMalloc(out, (size_t)bytes, hipHostMallocDefault));
    return PCS_OK;
}

int pcs_host_free(void *p) {
    if (p) HIPCHK(hipHostFree(p));
    return PCS_OK;
}

int pcs_membench(int device, int kind, int64_t bytes, int iters, int blocks_per_cu, float *mean_ms) {
    if (kind < 0 || kind > 8 || bytes < 4096 || iters < 1 || !mean_ms) return fail(PCS_ERR_ARG, "pcs_membench: bad arguments");
    if (device < 0 || device >= pcs_device_count()) return fail(PCS_ERR_NODEVICE, "pcs_membench: device %d not available", device);
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    void *src = nullptr, *dst = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto cleanup = [&]() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (src) (void)hipFree(src);
        if (dst) (void)hipFree(dst);
    };
#define MBCHK(expr)                                                                                              \
    do {                                                                                                         \
        hipError_t _e = (expr);                                                                                  \
        if (_e != hipSuccess) { const int _rc = fail(PCS_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); cleanup(); return _rc; } \
    } while (0)
    MBCHK(hipMalloc(&dst, bytes));
    if (kind == 2 || kind == 3) {
        MBCHK(hipMalloc(&src, bytes));
        MBCHK(hipMemset(src, 1, bytes));
    }
    MBCHK(hipEventCreate(&e0));
    MBCHK(hipEventCreate(&e1));
    const int64_t n16 = bytes / 16;
    const dim3 grid((unsigned)std::min<int64_t>((n16 + 255) / 256, (int64_t)prop.multiProcessorCount * std::max(1, blocks_per_cu)));
    void (*const kernels[9])(const double2 *, double2 *, int64_t) = {membench_kernel<0>, membench_kernel<1>, membench_kernel<2>, membench_kernel<3>, membench_kernel<4>,
                                                                    membench_kernel<5>, membench_kernel<6>, membench_kernel<7>, membench_kernel<8>};
    auto launch = [&]() { hipLaunchKernelGGL(kernels[kind], grid, dim3(256), 0, nullptr, (const double2 *)src, (double2 *)dst, n16); };
    for (int i = 0; i < 3; ++i) launch();
    MBCHK(hipEventRecord(e0, nullptr));
    for (int i = 0; i < iters; ++i) launch();
    MBCHK(hipEventRecord(e1, nullptr));
    MBCHK(hipEventSynchronize(e1));
    float ms = 0;
    MBCHK(hipEventElapsedTime(&ms, e0, e1));
#undef MBCHK
    *mean_ms = ms / iters;
    cleanup();
    return PCS_OK;
}
}  // extern "C"
