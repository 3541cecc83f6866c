// pcs_sweep.inc — host side of the plane-sweep depth (included by pcs_engine.hip behind pcs_fusion.inc; kernel: ba_sweep.hpp).  The handle
// owns the views as given (host), the neighbour lists, the warp table — 12 doubles per entry of the lists, formed here in FP64 when the
// lists are set — and the plane table of the last run.  Images and every output are the caller's device buffers; there is no workspace
// that grows with the images: the cost volume lives in registers and LDS.  Fence and timer are those of pcs_handle.inc.
// The views as given (host), the neighbour lists and the warp table: what pcs_sweep_set_views / pcs_sweep_set_neighbours keep, and
// pcs_pm_set_views / pcs_pm_set_neighbours (pcs_patchmatch.inc) with them.
struct RigViews {
    DevBuf nbr_start, nbr, warp;      // warp: double (entries, 12)
    std::vector<double> h_K, h_P;     // the views of set_views
    int64_t n_views = 0, n_nbr_views = -1;
    int width = 0, height = 0;
    bool ready() const { return n_views != 0 && n_nbr_views == n_views; }
};

struct pcs_plane_sweeper {
    HandleCore core;
    KernelTimer t_kernel;
    RigViews rig;
    DevBuf z;                         // double (n_z, D)
    std::vector<double> h_z;          // what z holds
};

static_assert(SWEEP_NOT_STRICT == PCS_SWEEP_NOT_STRICT && SWEEP_NO_VIEW == PCS_SWEEP_NO_VIEW && SWEEP_UNIQUENESS == PCS_SWEEP_UNIQUENESS, "status bits of pcs_hip.h");
static_assert(SWEEP_MAX_NBR == PCS_SWEEP_MAX_NEIGHBOURS && SWEEP_MAX_PLANES == PCS_SWEEP_MAX_PLANES, "limits of pcs_hip.h");
constexpr int SWEEP_DEFAULT_TW = 32;

// The warp of reference view i into neighbour j (include/pcs_hip.h, step 1): plain FP64 in the order written, sums left to right.
static void sweep_warp(const double *Ki, const double *Pi, const double *Kj, const double *Pj, double *out) {
#pragma clang fp contract(off)
    double M[9], c[3], N[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) M[3 * a + b] = (Pj[4 * a] * Pi[4 * b] + Pj[4 * a + 1] * Pi[4 * b + 1]) + Pj[4 * a + 2] * Pi[4 * b + 2];   // R_j R_i^T
    for (int a = 0; a < 3; ++a) c[a] = Pj[4 * a + 3] - ((M[3 * a] * Pi[3] + M[3 * a + 1] * Pi[7]) + M[3 * a + 2] * Pi[11]);
    for (int b = 0; b < 3; ++b) {   // N = K_j M
        N[b] = Kj[0] * M[b] + Kj[1] * M[6 + b];
        N[3 + b] = Kj[2] * M[3 + b] + Kj[3] * M[6 + b];
        N[6 + b] = M[6 + b];
    }
    for (int a = 0; a < 3; ++a) {   // A = N K_i^-1
        out[3 * a] = N[3 * a] / Ki[0];
        out[3 * a + 1] = N[3 * a + 1] / Ki[2];
        out[3 * a + 2] = (N[3 * a + 2] - out[3 * a] * Ki[1]) - out[3 * a + 1] * Ki[3];
    }
    out[9] = Kj[0] * c[0] + Kj[1] * c[2];
    out[10] = Kj[2] * c[1] + Kj[3] * c[2];
    out[11] = c[2];
}

// The bodies of set_views and set_neighbours of both handles; `r` NULL: the handle was.
static int rig_set_views(const char *who, RigViews *r, int64_t n_views, int width, int height, const double *K, const double *P) {
    if (const int rc = fuse_check_views(who, n_views, width, height, K, P)) return rc;
    if (!r) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    r->n_views = 0, r->n_nbr_views = -1;
    r->h_K.assign(K, K + 4 * n_views), r->h_P.assign(P, P + 12 * n_views);
    r->n_views = n_views, r->width = width, r->height = height;
    return PCS_OK;
}

static int rig_set_neighbours(const char *who, const char *views_first, RigViews *r, const HandleCore *core, const int32_t *nbr_start, const int32_t *nbr, int64_t n) {
    if (const int rc = fuse_check_neighbours(who, nbr_start, nbr, n, SWEEP_MAX_NBR)) return rc;
    if (!r) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (r->n_views == 0) return fail(PCS_ERR_STATE, "%s: %s comes first", who, views_first);
    if (n != r->n_views) return fail(PCS_ERR_ARG, "%s: n %lld differs from the %lld views of %s", who, (long long)n, (long long)r->n_views, views_first);
    std::vector<double> warp(12 * (size_t)nbr_start[n]);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t e = nbr_start[i]; e < nbr_start[i + 1]; ++e)
            sweep_warp(&r->h_K[4 * i], &r->h_P[12 * i], &r->h_K[4 * (size_t)nbr[e]], &r->h_P[12 * (size_t)nbr[e]], &warp[12 * (size_t)e]);
    HIPCHK(core->quiesce());   // a queued run may still read the old tables
    r->n_nbr_views = -1;
    const HostArray up[] = {{r->nbr_start, nbr_start, n + 1, sizeof(int32_t)}, {r->nbr, nbr, nbr_start[n], sizeof(int32_t)}, {r->warp, warp.data(), 12 * (int64_t)nbr_start[n], sizeof(double)}};
    if (const int rc = upload_host_arrays(*core, up, 3)) return rc;
    r->n_nbr_views = n;
    return PCS_OK;
}

// Every argument of pcs_sweep_run but the handle: nothing here touches the device.
static int sweep_check_run(const char *who, const void *d_images, const double *z, int64_t n_z, int D, int census_w, int census_h, int box_radius, int truncate,
                           int uniqueness_ratio, const void *d_depth, int depth_dtype) {
    if (!d_images) return fail(PCS_ERR_ARG, "%s: d_images must be given", who);
    if (n_z < 1 || n_z > STEREO_MAX_PAIRS) return fail(PCS_ERR_ARG, "%s: n_z %lld must be 1 or the number of views", who, (long long)n_z);
    if (D < 1 || D > SWEEP_MAX_PLANES) return fail(PCS_ERR_ARG, "%s: D %d outside [1, %d]", who, D, SWEEP_MAX_PLANES);
    if (!z) return fail(PCS_ERR_ARG, "%s: z (n_z, D) must be given", who);
    for (int64_t v = 0; v < n_z; ++v) {
        const double *row = z + v * D;
        for (int k = 0; k < D; ++k)
            if (!std::isfinite(row[k]) || !(row[k] > 0.0)) return fail(PCS_ERR_ARG, "%s: z of row %lld, plane %d must be finite and > 0 (got %g)", who, (long long)v, k, row[k]);
        for (int k = 1; k < D; ++k)
            if (row[k] == row[k - 1] || (row[k] > row[k - 1]) != (row[1] > row[0]))
                return fail(PCS_ERR_ARG, "%s: z of row %lld must be strictly monotone (plane %d)", who, (long long)v, k);
    }
    if (census_w < 3 || census_w % 2 == 0) return fail(PCS_ERR_ARG, "%s: census_w %d must be odd and >= 3", who, census_w);
    if (census_h < 3 || census_h % 2 == 0) return fail(PCS_ERR_ARG, "%s: census_h %d must be odd and >= 3", who, census_h);
    if ((int64_t)census_w * census_h - 1 > SGM_MAX_BITS)
        return fail(PCS_ERR_ARG, "%s: the census window %d x %d has %lld bits, more than %d", who, census_w, census_h, (long long)census_w * census_h - 1, SGM_MAX_BITS);
    if (box_radius < 0 || box_radius > SWEEP_MAX_BOX) return fail(PCS_ERR_ARG, "%s: box_radius %d outside [0, %d]", who, box_radius, SWEEP_MAX_BOX);
    const int full = (census_w * census_h - 1) * (2 * box_radius + 1) * (2 * box_radius + 1);
    if (truncate < 1 || truncate > full) return fail(PCS_ERR_ARG, "%s: truncate %d outside [1, %d]", who, truncate, full);
    if (uniqueness_ratio < 0 || uniqueness_ratio > 100) return fail(PCS_ERR_ARG, "%s: uniqueness_ratio %d outside [0, 100]", who, uniqueness_ratio);
    if (depth_dtype != PCS_F64 && depth_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: depth_dtype PCS_F64 or PCS_F32", who);
    if (!d_depth) return fail(PCS_ERR_ARG, "%s: d_depth must be given", who);
    return PCS_OK;
}

extern "C" {
int pcs_sweep_create(pcs_plane_sweeper **out, int device) {
    if (!out) return fail(PCS_ERR_ARG, "pcs_sweep_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_sweep_create", device)) return rc;
    pcs_plane_sweeper *p = new pcs_plane_sweeper();
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->t_kernel.create();
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_sweep_create: %s", hipGetErrorString(e));
        pcs_sweep_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_sweep_destroy(pcs_plane_sweeper *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->rig.nbr_start, &p->rig.nbr, &p->rig.warp, &p->z}, {&p->t_kernel});
    delete p;
    return PCS_OK;
}

// K and P are HOST arrays and are copied.  New views drop the neighbour lists and with them the warp table.
int pcs_sweep_set_views(pcs_plane_sweeper *p, int64_t n_views, int width, int height, const double *K, const double *P) {
    return rig_set_views("pcs_sweep_set_views", p ? &p->rig : nullptr, n_views, width, height, K, P);
}

int pcs_sweep_set_neighbours(pcs_plane_sweeper *p, const int32_t *nbr_start, const int32_t *nbr, int64_t n) {
    return rig_set_neighbours("pcs_sweep_set_neighbours", "pcs_sweep_set_views", p ? &p->rig : nullptr, p ? &p->core : nullptr, nbr_start, nbr, n);
}

// z is a HOST table; it is uploaded when it differs from what the handle holds.
int pcs_sweep_run(pcs_plane_sweeper *p, const uint8_t *d_images, int64_t pitch, const double *z, int64_t n_z, int D, int census_w, int census_h, int box_radius, int truncate,
                  int uniqueness_ratio, void *d_depth, int depth_dtype, int32_t *d_level, int32_t *d_cost, uint8_t *d_status, void *stream) {
    const char *who = "pcs_sweep_run";
    if (const int rc = sweep_check_run(who, d_images, z, n_z, D, census_w, census_h, box_radius, truncate, uniqueness_ratio, d_depth, depth_dtype)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (!p->rig.ready()) return fail(PCS_ERR_STATE, "%s: pcs_sweep_set_views and pcs_sweep_set_neighbours come first", who);
    if (n_z != 1 && n_z != p->rig.n_views) return fail(PCS_ERR_ARG, "%s: n_z %lld must be 1 or the %lld views", who, (long long)n_z, (long long)p->rig.n_views);
    if (pitch < p->rig.width) return fail(PCS_ERR_ARG, "%s: pitch %lld is below the row size %d", who, (long long)pitch, p->rig.width);
    int tw = stereo_env_int("PCS_SWEEP_TILE_COLUMNS", 8, 64);   // measurements, and the test of "any tiling gives the same bits"
    if (tw != 8 && tw != 16 && tw != 32 && tw != 64) tw = SWEEP_DEFAULT_TW;
    const int th = SWEEP_PPT * SWEEP_THREADS / tw;
    const std::vector<double> zt(z, z + n_z * D);
    const bool upload = zt != p->h_z;
    HIPCHK(hipSetDevice(p->core.device));
    if (upload) {
        HIPCHK(p->core.quiesce());   // a queued run may still read the old planes
        p->h_z.clear();
    }
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, upload && p->z.grows((int64_t)zt.size())));
    if (upload) {
        if (const int rc = p->z.grow((int64_t)zt.size(), sizeof(double))) return rc;
        HIPCHK(hipMemcpy(p->z.p, zt.data(), sizeof(double) * zt.size(), hipMemcpyHostToDevice));
        p->h_z = zt;
    }
    SweepArgs a{};
    a.images = d_images, a.pitch = pitch, a.warp = p->rig.warp.as<const double>(), a.nbr_start = p->rig.nbr_start.as<const int32_t>(), a.nbr = p->rig.nbr.as<const int32_t>();
    a.z = p->z.as<const double>(), a.z_stride = n_z == 1 ? 0 : D, a.D = D, a.W = p->rig.width, a.H = p->rig.height;
    a.rw = census_w / 2, a.rh = census_h / 2, a.r = box_radius, a.tau = truncate, a.uniq = uniqueness_ratio;
    a.tw_log2 = tw == 8 ? 3 : tw == 16 ? 4 : tw == 32 ? 5 : 6;
    a.depth = d_depth, a.depth_f32 = depth_dtype == PCS_F32, a.level = d_level, a.cost = d_cost, a.status = d_status;
    const dim3 grid((unsigned)((a.W + tw - 1) / tw), (unsigned)((a.H + th - 1) / th), (unsigned)p->rig.n_views);
    const size_t lds = (size_t)sweep_lds_bytes(tw, a.rw, a.rh, a.r);   // below 32 KiB at every admitted tile, window and box
    HIPCHK(hipEventRecord(p->t_kernel.e0, s));
    hipLaunchKernelGGL(sweep_kernel, grid, dim3(SWEEP_THREADS), lds, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_kernel.e1, s));
    p->t_kernel.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_sweep_last_kernel_ms(pcs_plane_sweeper *p, float *kernel_ms) {
    const char *who = "pcs_sweep_last_kernel_ms";
    if (!p) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    return timer_ms(who, &p->t_kernel, kernel_ms, "nothing has run yet");
}

}  // extern "C"
