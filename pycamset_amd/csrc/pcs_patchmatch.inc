// pcs_patchmatch.inc — host side of the PatchMatch depth (included by pcs_engine.hip behind pcs_sweep.inc; kernels: ba_patchmatch.hpp).
// The handle owns what the sweep's handle owns of a rig (RigViews of pcs_sweep.inc: the views as given, the neighbour lists, the warp
// table) and a small per-view table: inverse-depth bounds, slope bound, intrinsics.  Images, planes, costs and every output are the
// caller's device buffers; the state is used in place and nothing here grows with the images.
struct pcs_patchmatch {
    HandleCore core;
    KernelTimer t_kernel;
    RigViews rig;
    DevBuf view;                  // double (V, PM_VIEW_WORDS)
    std::vector<double> h_view;   // what view holds
};

static_assert(PM_NOT_STRICT == PCS_PM_NOT_STRICT && PM_NO_VIEW == PCS_PM_NO_VIEW && PM_MAX_NBR == PCS_PM_MAX_NEIGHBOURS && PM_MAX_NBR == SWEEP_MAX_NBR, "pcs_hip.h");
constexpr int PM_DEFAULT_TW = 32;

// What init, iterate and finish share of their arguments: nothing here touches the device.
static int pm_check_window(const char *who, int census_w, int census_h, int stride, int truncate) {
    if (census_w < 3 || census_w % 2 == 0) return fail(PCS_ERR_ARG, "%s: census_w %d must be odd and >= 3", who, census_w);
    if (census_h < 3 || census_h % 2 == 0) return fail(PCS_ERR_ARG, "%s: census_h %d must be odd and >= 3", who, census_h);
    if ((int64_t)census_w * census_h - 1 > SGM_MAX_BITS)
        return fail(PCS_ERR_ARG, "%s: the census window %d x %d has %lld bits, more than %d", who, census_w, census_h, (long long)census_w * census_h - 1, SGM_MAX_BITS);
    if (stride < 1 || stride > PM_MAX_STRIDE) return fail(PCS_ERR_ARG, "%s: stride %d outside [1, %d]", who, stride, PM_MAX_STRIDE);
    if (truncate < 1 || truncate > census_w * census_h - 1) return fail(PCS_ERR_ARG, "%s: truncate %d outside [1, %d]", who, truncate, census_w * census_h - 1);
    return PCS_OK;
}

static int pm_check_search(const char *who, const void *d_images, const double *wrange, int64_t n_w, const double *slope_max, int census_w, int census_h, int stride,
                           int truncate, const void *d_plane, const void *d_cost) {
    if (!d_images) return fail(PCS_ERR_ARG, "%s: d_images must be given", who);
    if (n_w < 1 || n_w > STEREO_MAX_PAIRS) return fail(PCS_ERR_ARG, "%s: n_w %lld must be 1 or the number of views", who, (long long)n_w);
    if (!wrange) return fail(PCS_ERR_ARG, "%s: wrange (n_w, 2) must be given", who);
    for (int64_t v = 0; v < n_w; ++v)
        if (!std::isfinite(wrange[2 * v]) || !std::isfinite(wrange[2 * v + 1]) || !(wrange[2 * v] > 0.0) || !(wrange[2 * v] < wrange[2 * v + 1]))
            return fail(PCS_ERR_ARG, "%s: wrange of row %lld must be finite with 0 < w_lo < w_hi (got %g, %g)", who, (long long)v, wrange[2 * v], wrange[2 * v + 1]);
    if (!slope_max) return fail(PCS_ERR_ARG, "%s: slope_max (n_views) must be given", who);
    if (const int rc = pm_check_window(who, census_w, census_h, stride, truncate)) return rc;
    if (!d_plane) return fail(PCS_ERR_ARG, "%s: d_plane must be given", who);
    if (!d_cost) return fail(PCS_ERR_ARG, "%s: d_cost must be given", who);
    return PCS_OK;
}

// Behind the checks: the handle, the per-view table (uploaded when it differs from what the handle holds) and the arguments every kernel
// reads.  `wrange` NULL (finish): the table is left as the last init or iterate made it.
static int pm_prepare(const char *who, pcs_patchmatch *p, const uint8_t *d_images, int64_t pitch, const double *wrange, int64_t n_w, const double *slope_max, int census_w,
                      int census_h, int stride, int truncate, void *stream, hipStream_t *s_out, PmArgs *a) {
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (!p->rig.ready()) return fail(PCS_ERR_STATE, "%s: pcs_pm_set_views and pcs_pm_set_neighbours come first", who);
    const int64_t V = p->rig.n_views;
    std::vector<double> vt;
    if (wrange) {
        if (n_w != 1 && n_w != V) return fail(PCS_ERR_ARG, "%s: n_w %lld must be 1 or the %lld views", who, (long long)n_w, (long long)V);
        if (pitch < p->rig.width) return fail(PCS_ERR_ARG, "%s: pitch %lld is below the row size %d", who, (long long)pitch, p->rig.width);
        for (int64_t v = 0; v < V; ++v)
            if (!std::isfinite(slope_max[v]) || !(slope_max[v] > 0.0)) return fail(PCS_ERR_ARG, "%s: slope_max of view %lld must be finite and > 0 (got %g)", who, (long long)v, slope_max[v]);
        vt.resize((size_t)V * PM_VIEW_WORDS);
        for (int64_t v = 0; v < V; ++v) {
            const double *r = wrange + 2 * (n_w == 1 ? 0 : v), *K = &p->rig.h_K[4 * v];
            const double row[PM_VIEW_WORDS] = {r[0], r[1], slope_max[v], K[0], K[1], K[2], K[3], 0.0};
            std::copy(row, row + PM_VIEW_WORDS, &vt[(size_t)v * PM_VIEW_WORDS]);
        }
    } else if (p->h_view.size() != (size_t)V * PM_VIEW_WORDS)
        return fail(PCS_ERR_STATE, "%s: pcs_pm_init or pcs_pm_iterate comes first", who);
    const bool upload = wrange && vt != p->h_view;
    HIPCHK(hipSetDevice(p->core.device));
    if (upload) {
        HIPCHK(p->core.quiesce());   // a queued run may still read the old table
        p->h_view.clear();
    }
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, upload && p->view.grows((int64_t)vt.size())));
    if (upload) {
        if (const int rc = p->view.grow((int64_t)vt.size(), sizeof(double))) return rc;
        HIPCHK(hipMemcpy(p->view.p, vt.data(), sizeof(double) * vt.size(), hipMemcpyHostToDevice));
        p->h_view = vt;
    }
    *a = PmArgs{};
    a->images = d_images, a->pitch = pitch, a->warp = p->rig.warp.as<const double>(), a->nbr_start = p->rig.nbr_start.as<const int32_t>(), a->nbr = p->rig.nbr.as<const int32_t>();
    a->view = p->view.as<const double>(), a->W = p->rig.width, a->H = p->rig.height;
    a->rw = census_w / 2, a->rh = census_h / 2, a->stride = stride, a->tau = truncate;
    *s_out = s;
    return PCS_OK;
}

static dim3 pm_pixel_grid(const pcs_patchmatch *p) {   // pm_init_kernel and pm_finish_kernel: 64 x 4 pixels per workgroup
    return dim3((unsigned)((p->rig.width + 63) / 64), (unsigned)((p->rig.height + 3) / 4), (unsigned)p->rig.n_views);
}

extern "C" {
int pcs_pm_create(pcs_patchmatch **out, int device) {
    if (!out) return fail(PCS_ERR_ARG, "pcs_pm_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_pm_create", device)) return rc;
    pcs_patchmatch *p = new pcs_patchmatch();
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->t_kernel.create();
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_pm_create: %s", hipGetErrorString(e));
        pcs_pm_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_pm_destroy(pcs_patchmatch *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->rig.nbr_start, &p->rig.nbr, &p->rig.warp, &p->view}, {&p->t_kernel});
    delete p;
    return PCS_OK;
}

int pcs_pm_set_views(pcs_patchmatch *p, int64_t n_views, int width, int height, const double *K, const double *P) {
    const int rc = rig_set_views("pcs_pm_set_views", p ? &p->rig : nullptr, n_views, width, height, K, P);
    if (rc == PCS_OK) p->h_view.clear();   // the table holds the intrinsics
    return rc;
}

int pcs_pm_set_neighbours(pcs_patchmatch *p, const int32_t *nbr_start, const int32_t *nbr, int64_t n) {
    return rig_set_neighbours("pcs_pm_set_neighbours", "pcs_pm_set_views", p ? &p->rig : nullptr, p ? &p->core : nullptr, nbr_start, nbr, n);
}

int pcs_pm_init(pcs_patchmatch *p, const uint8_t *d_images, int64_t pitch, const double *wrange, int64_t n_w, const double *slope_max, int census_w, int census_h, int stride,
                int truncate, uint64_t seed, const void *d_start_depth, int start_dtype, int start_planes, double *d_plane, int32_t *d_cost, void *stream) {
    const char *who = "pcs_pm_init";
    if (const int rc = pm_check_search(who, d_images, wrange, n_w, slope_max, census_w, census_h, stride, truncate, d_plane, d_cost)) return rc;
    if (d_start_depth && start_dtype != PCS_F64 && start_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: start_dtype PCS_F64 or PCS_F32", who);
    if (start_planes != 0 && start_planes != 1) return fail(PCS_ERR_ARG, "%s: start_planes %d must be 0 or 1", who, start_planes);
    if (start_planes && d_start_depth) return fail(PCS_ERR_ARG, "%s: d_start_depth and start_planes exclude each other", who);
    PmArgs a;
    hipStream_t s;
    if (const int rc = pm_prepare(who, p, d_images, pitch, wrange, n_w, slope_max, census_w, census_h, stride, truncate, stream, &s, &a)) return rc;
    a.seed = seed, a.plane = d_plane, a.cost = d_cost, a.start_depth = d_start_depth, a.start_f32 = start_dtype == PCS_F32, a.start_planes = start_planes;
    HIPCHK(hipEventRecord(p->t_kernel.e0, s));
    hipLaunchKernelGGL(pm_init_kernel, pm_pixel_grid(p), dim3(PM_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_kernel.e1, s));
    p->t_kernel.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

// Iterations first_iteration .. first_iteration + n_iterations - 1, two launches each; n_iterations = 0 launches nothing.
int pcs_pm_iterate(pcs_patchmatch *p, int first_iteration, int n_iterations, const uint8_t *d_images, int64_t pitch, const double *wrange, int64_t n_w, const double *slope_max,
                   int census_w, int census_h, int stride, int truncate, uint64_t seed, double *d_plane, int32_t *d_cost, void *stream) {
    const char *who = "pcs_pm_iterate";
    if (first_iteration < 0 || first_iteration > PM_MAX_ITERATION) return fail(PCS_ERR_ARG, "%s: first_iteration %d outside [0, %d]", who, first_iteration, PM_MAX_ITERATION);
    if (n_iterations < 0 || n_iterations > PM_MAX_ITERATION - first_iteration)
        return fail(PCS_ERR_ARG, "%s: n_iterations %d outside [0, %d - first_iteration]", who, n_iterations, PM_MAX_ITERATION);
    if (const int rc = pm_check_search(who, d_images, wrange, n_w, slope_max, census_w, census_h, stride, truncate, d_plane, d_cost)) return rc;
    PmArgs a;
    hipStream_t s;
    if (const int rc = pm_prepare(who, p, d_images, pitch, wrange, n_w, slope_max, census_w, census_h, stride, truncate, stream, &s, &a)) return rc;
    int tw = stereo_env_int("PCS_PM_TILE_COLUMNS", 8, 64);   // measurements, and the test of "any tiling gives the same bits"
    if (tw != 8 && tw != 16 && tw != 32 && tw != 64) tw = PM_DEFAULT_TW;
    const int th = PM_TILE_PIXELS / tw;
    a.seed = seed, a.plane = d_plane, a.cost = d_cost, a.tw_log2 = tw == 8 ? 3 : tw == 16 ? 4 : tw == 32 ? 5 : 6;
    const dim3 grid((unsigned)((a.W + tw - 1) / tw), (unsigned)((a.H + th - 1) / th), (unsigned)p->rig.n_views);
    HIPCHK(hipEventRecord(p->t_kernel.e0, s));
    for (int it = first_iteration; it < first_iteration + n_iterations; ++it)
        for (int colour = 0; colour < 2; ++colour) {
            a.it = it, a.colour = colour, a.rho = std::ldexp(1.0, -(2 + it)), a.half_it = std::ldexp(1.0, -(1 + it));
            hipLaunchKernelGGL(pm_half_kernel, grid, dim3(PM_THREADS), 0, s, a);
        }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_kernel.e1, s));
    p->t_kernel.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_pm_finish(pcs_patchmatch *p, int census_w, int census_h, int stride, int truncate, const double *d_plane, const int32_t *d_cost, void *d_depth, int depth_dtype,
                  void *d_normal, uint8_t *d_status, void *stream) {
    const char *who = "pcs_pm_finish";
    if (const int rc = pm_check_window(who, census_w, census_h, stride, truncate)) return rc;
    if (!d_plane) return fail(PCS_ERR_ARG, "%s: d_plane must be given", who);
    if (!d_cost) return fail(PCS_ERR_ARG, "%s: d_cost must be given", who);
    if (depth_dtype != PCS_F64 && depth_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: depth_dtype PCS_F64 or PCS_F32", who);
    if (!d_depth) return fail(PCS_ERR_ARG, "%s: d_depth must be given", who);
    PmArgs a;
    hipStream_t s;
    if (const int rc = pm_prepare(who, p, nullptr, 0, nullptr, 0, nullptr, census_w, census_h, stride, truncate, stream, &s, &a)) return rc;
    a.plane = const_cast<double *>(d_plane), a.cost = const_cast<int32_t *>(d_cost), a.depth = d_depth, a.normal = d_normal, a.out_f32 = depth_dtype == PCS_F32, a.status = d_status;
    HIPCHK(hipEventRecord(p->t_kernel.e0, s));
    hipLaunchKernelGGL(pm_finish_kernel, pm_pixel_grid(p), dim3(PM_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_kernel.e1, s));
    p->t_kernel.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_pm_last_kernel_ms(pcs_patchmatch *p, float *kernel_ms) {
    const char *who = "pcs_pm_last_kernel_ms";
    if (!p) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    return timer_ms(who, &p->t_kernel, kernel_ms, "nothing has run yet");
}

}  // extern "C"
