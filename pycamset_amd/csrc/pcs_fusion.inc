// pcs_fusion.inc — host side of the depth-map fusion (included by pcs_engine.hip behind pcs_stereo.inc; kernels: ba_fusion.hpp).  The handle
// owns the view table (16 doubles per view), the neighbour lists, the transform of the last run and the workspace: the support words
// when the caller does not ask for them, and the block counts and offsets of the per-view counts (the compaction's own kernels,
// stereo_count_kernel / stereo_scan_kernel, run on the final mask).  Depth maps and every output are the caller's device buffers.
// Fence and timers are those of pcs_handle.inc (DESIGN.md, "Batched handles").
struct pcs_depth_fuser {
    HandleCore core;
    KernelTimer t_check, t_unique, t_total;
    DevBuf views, nbr_start, nbr, support, blk, off, tf;   // views: double (V, 16); support: uint32 (V, H, W); tf: double (12)
    std::vector<double> h_tf;                              // what tf holds
    int64_t n_views = 0, n_nbr_views = -1;                 // n_nbr_views: the views the neighbour lists were checked for (-1: none set)
    int width = 0, height = 0;
    bool ran_unique = false;
};

static_assert(FUSE_INVALID == PCS_FUSE_INVALID_DEPTH && FUSE_FEW == PCS_FUSE_FEW_VIEWS && FUSE_DUPLICATE == PCS_FUSE_DUPLICATE, "status bits of pcs_hip.h");
static_assert(FUSE_MAX_NBR == PCS_FUSE_MAX_NEIGHBOURS, "the width of the support word");

// Every argument of pcs_fuse_set_views but the handle: nothing here touches the device.
static int fuse_check_views(const char *who, int64_t n_views, int width, int height, const double *K, const double *P) {
    if (const int rc = stereo_check_shape(who, n_views, width, height)) return rc;   // the compaction's limits: it follows unchanged
    if (n_views < 1) return fail(PCS_ERR_ARG, "%s: n_views %lld must be at least 1", who, (long long)n_views);
    if (!K) return fail(PCS_ERR_ARG, "%s: K (n_views, 4) = [fx, cx, fy, cy] must be given", who);
    if (!P) return fail(PCS_ERR_ARG, "%s: P (n_views, 12) = [R | t] world -> view must be given", who);
    for (int64_t v = 0; v < n_views; ++v) {
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(K[4 * v + k])) return fail(PCS_ERR_ARG, "%s: K of view %lld is not finite", who, (long long)v);
        if (K[4 * v] == 0.0 || K[4 * v + 2] == 0.0) return fail(PCS_ERR_ARG, "%s: K of view %lld has a focal length of 0", who, (long long)v);
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(P[12 * v + k])) return fail(PCS_ERR_ARG, "%s: P of view %lld is not finite", who, (long long)v);
    }
    return PCS_OK;
}

// The device's view table: per view K = [fx, cx, fy, cy], then the 3 x 4 [R | t] row-major (16 doubles; also pcs_tsdf_set_views)
static std::vector<double> fuse_view_rows(int64_t n_views, const double *K, const double *P) {
    std::vector<double> rows(16 * (size_t)n_views);
    for (int64_t v = 0; v < n_views; ++v) {
        std::copy(K + 4 * v, K + 4 * v + 4, rows.begin() + 16 * v);
        std::copy(P + 12 * v, P + 12 * v + 12, rows.begin() + 16 * v + 4);
    }
    return rows;
}

// Every argument of pcs_fuse_set_neighbours but the handle (and of pcs_sweep_set_neighbours, whose lists hold at most `cap` = 16).
static int fuse_check_neighbours(const char *who, const int32_t *nbr_start, const int32_t *nbr, int64_t n, int cap = FUSE_MAX_NBR) {
    if (n < 1 || n > STEREO_MAX_PAIRS) return fail(PCS_ERR_ARG, "%s: n %lld outside [1, %lld]", who, (long long)n, (long long)STEREO_MAX_PAIRS);
    if (!nbr_start) return fail(PCS_ERR_ARG, "%s: nbr_start (n + 1) must be given", who);
    if (nbr_start[0] != 0) return fail(PCS_ERR_ARG, "%s: nbr_start must begin at 0 (got %d)", who, nbr_start[0]);
    for (int64_t v = 0; v < n; ++v) {
        const int64_t len = (int64_t)nbr_start[v + 1] - nbr_start[v];
        if (len < 0) return fail(PCS_ERR_ARG, "%s: nbr_start must be non-decreasing (view %lld)", who, (long long)v);
        if (len > cap) return fail(PCS_ERR_ARG, "%s: nbr_start gives view %lld %lld neighbours, more than %d", who, (long long)v, (long long)len, cap);
    }
    if (nbr_start[n] > 0 && !nbr) return fail(PCS_ERR_ARG, "%s: nbr must be given", who);
    for (int64_t v = 0; v < n; ++v)
        for (int32_t a = nbr_start[v]; a < nbr_start[v + 1]; ++a) {
            if (nbr[a] < 0 || nbr[a] >= n) return fail(PCS_ERR_ARG, "%s: nbr entry %d of view %lld is %d, outside [0, %lld)", who, a - nbr_start[v], (long long)v, nbr[a], (long long)n);
            if (nbr[a] == v) return fail(PCS_ERR_ARG, "%s: nbr lists view %lld as its own neighbour", who, (long long)v);
            for (int32_t b = nbr_start[v]; b < a; ++b)
                if (nbr[b] == nbr[a]) return fail(PCS_ERR_ARG, "%s: nbr lists view %d twice for view %lld", who, nbr[a], (long long)v);
        }
    return PCS_OK;
}

// Every argument of pcs_fuse_run but the handle.
static int fuse_check_run(const char *who, const void *d_depth, int depth_dtype, double px_tol, double rel_tol, int min_views, int unique, const double *T, const void *d_points,
                          int points_dtype, const void *d_mask, const void *d_fused_depth, int fused_dtype) {
    if (depth_dtype != PCS_F64 && depth_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: depth_dtype PCS_F64 or PCS_F32", who);
    if (!std::isfinite(px_tol) || !(px_tol > 0.0)) return fail(PCS_ERR_ARG, "%s: px_tol must be finite and > 0 (got %g)", who, px_tol);
    if (!std::isfinite(rel_tol) || !(rel_tol > 0.0)) return fail(PCS_ERR_ARG, "%s: rel_tol must be finite and > 0 (got %g)", who, rel_tol);
    if (min_views < 1 || min_views > FUSE_MAX_NBR) return fail(PCS_ERR_ARG, "%s: min_views %d outside [1, %d]", who, min_views, FUSE_MAX_NBR);
    if (unique != 0 && unique != 1) return fail(PCS_ERR_ARG, "%s: unique %d must be 0 or 1", who, unique);
    for (int k = 0; T && k < 12; ++k)
        if (!std::isfinite(T[k])) return fail(PCS_ERR_ARG, "%s: T is not finite", who);
    if (points_dtype != PCS_F64 && points_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: points_dtype PCS_F64 or PCS_F32", who);
    if (d_fused_depth && fused_dtype != PCS_F64 && fused_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: fused_dtype PCS_F64 or PCS_F32", who);
    if (!d_depth) return fail(PCS_ERR_ARG, "%s: d_depth must be given", who);
    if (!d_points || !d_mask) return fail(PCS_ERR_ARG, "%s: d_points and d_mask must be given", who);
    return PCS_OK;
}

template <class T>
static void fuse_launch(const FuseArgs &a, int64_t n_views, bool unique, pcs_depth_fuser *p, hipStream_t s) {
    const dim3 grid((unsigned)((a.W + FUSE_TX - 1) / FUSE_TX), (unsigned)((a.H + FUSE_TY - 1) / FUSE_TY), (unsigned)n_views), block(FUSE_TX, FUSE_TY);
    (void)hipEventRecord(p->t_check.e0, s);
    hipLaunchKernelGGL(fuse_check_kernel<T>, grid, block, 0, s, a);
    (void)hipEventRecord(p->t_check.e1, s);
    if (!unique) return;
    (void)hipEventRecord(p->t_unique.e0, s);
    hipLaunchKernelGGL(fuse_unique_kernel<T>, grid, block, 0, s, a);
    (void)hipEventRecord(p->t_unique.e1, s);
}

extern "C" {
int pcs_fuse_create(pcs_depth_fuser **out, int device) {
    if (!out) return fail(PCS_ERR_ARG, "pcs_fuse_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_fuse_create", device)) return rc;
    pcs_depth_fuser *p = new pcs_depth_fuser();
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->t_check.create();
    if (e == hipSuccess) e = p->t_unique.create();
    if (e == hipSuccess) e = p->t_total.create();
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_fuse_create: %s", hipGetErrorString(e));
        pcs_fuse_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_fuse_destroy(pcs_depth_fuser *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->views, &p->nbr_start, &p->nbr, &p->support, &p->blk, &p->off, &p->tf}, {&p->t_check, &p->t_unique, &p->t_total});
    delete p;
    return PCS_OK;
}

// K and P are HOST arrays and are copied.  New views drop the neighbour lists: they were checked against the old number of views.
int pcs_fuse_set_views(pcs_depth_fuser *p, int64_t n_views, int width, int height, const double *K, const double *P) {
    const char *who = "pcs_fuse_set_views";
    if (const int rc = fuse_check_views(who, n_views, width, height, K, P)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    const std::vector<double> rows = fuse_view_rows(n_views, K, P);
    HIPCHK(p->core.quiesce());   // a queued run may still read the old table
    p->n_views = 0, p->n_nbr_views = -1;
    const HostArray up[] = {{p->views, rows.data(), 16 * n_views, sizeof(double)}};
    if (const int rc = upload_host_arrays(p->core, up, 1)) return rc;
    p->n_views = n_views, p->width = width, p->height = height;
    return PCS_OK;
}

int pcs_fuse_set_neighbours(pcs_depth_fuser *p, const int32_t *nbr_start, const int32_t *nbr, int64_t n) {
    const char *who = "pcs_fuse_set_neighbours";
    if (const int rc = fuse_check_neighbours(who, nbr_start, nbr, n)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (p->n_views == 0) return fail(PCS_ERR_STATE, "%s: pcs_fuse_set_views comes first", who);
    if (n != p->n_views) return fail(PCS_ERR_ARG, "%s: n %lld differs from the %lld views of pcs_fuse_set_views", who, (long long)n, (long long)p->n_views);
    HIPCHK(p->core.quiesce());
    p->n_nbr_views = -1;
    const HostArray up[] = {{p->nbr_start, nbr_start, n + 1, sizeof(int32_t)}, {p->nbr, nbr, nbr_start[n], sizeof(int32_t)}};
    if (const int rc = upload_host_arrays(p->core, up, 2)) return rc;
    p->n_nbr_views = n;
    return PCS_OK;
}

// T is a HOST array; it is uploaded when it differs from what the handle holds.
int pcs_fuse_run(pcs_depth_fuser *p, const void *d_depth, int depth_dtype, double px_tol, double rel_tol, int min_views, int unique, const double *T, void *d_points,
                 int points_dtype, uint8_t *d_mask, uint8_t *d_count, uint32_t *d_support, uint8_t *d_status, void *d_fused_depth, int fused_dtype, int64_t *d_counts,
                 void *stream) {
    const char *who = "pcs_fuse_run";
    if (const int rc = fuse_check_run(who, d_depth, depth_dtype, px_tol, rel_tol, min_views, unique, T, d_points, points_dtype, d_mask, d_fused_depth, fused_dtype)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (p->n_views == 0 || p->n_nbr_views != p->n_views) return fail(PCS_ERR_STATE, "%s: pcs_fuse_set_views and pcs_fuse_set_neighbours come first", who);
    const int64_t n = p->n_views, npix = n * p->height * p->width;
    const int64_t nblk = stereo_blocks_per_pair(p->width, p->height), NB = n * nblk;
    const std::vector<double> tf = T ? std::vector<double>(T, T + 12) : std::vector<double>();
    const bool upload = T && tf != p->h_tf;
    const bool grows = (upload && p->tf.grows(12)) || (!d_support && p->support.grows(npix)) || (d_counts && (p->blk.grows(NB) || p->off.grows(NB + 1)));
    HIPCHK(hipSetDevice(p->core.device));
    if (upload) {
        HIPCHK(p->core.quiesce());   // a queued run may still read the old transform
        p->h_tf.clear();
    }
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));
    if (upload) {
        if (const int rc = p->tf.grow(12, sizeof(double))) return rc;
        HIPCHK(hipMemcpy(p->tf.p, tf.data(), sizeof(double) * 12, hipMemcpyHostToDevice));
        p->h_tf = tf;
    }
    if (!d_support)
        if (const int rc = p->support.grow(npix, sizeof(uint32_t))) return rc;
    if (d_counts) {
        if (const int rc = p->blk.grow(NB, sizeof(int32_t))) return rc;
        if (const int rc = p->off.grow(NB + 1, sizeof(int64_t))) return rc;
    }
    FuseArgs a{};
    a.views = p->views.as<const double>(), a.nbr_start = p->nbr_start.as<const int32_t>(), a.nbr = p->nbr.as<const int32_t>(), a.depth = d_depth;
    a.W = p->width, a.H = p->height, a.min_views = min_views, a.px_tol2 = px_tol * px_tol, a.rel_tol = rel_tol, a.T = T ? p->tf.as<const double>() : nullptr;
    a.pts = d_points, a.f32 = points_dtype == PCS_F32, a.mask = d_mask, a.count = d_count, a.status = d_status;
    a.support = d_support ? d_support : p->support.as<uint32_t>(), a.fused = d_fused_depth, a.fused_f32 = fused_dtype == PCS_F32;
    HIPCHK(hipEventRecord(p->t_total.e0, s));
    if (depth_dtype == PCS_F32) fuse_launch<float>(a, n, unique != 0, p, s);
    else fuse_launch<double>(a, n, unique != 0, p, s);
    if (d_counts) {
        hipLaunchKernelGGL(stereo_count_kernel, dim3((unsigned)nblk, (unsigned)n), dim3(STEREO_PIX_PER_BLOCK), 0, s, (const uint8_t *)d_mask, (int64_t)p->width * p->height, (int)nblk,
                           p->blk.as<int32_t>());
        hipLaunchKernelGGL(stereo_scan_kernel, dim3(1), dim3(1024), 0, s, p->blk.as<const int32_t>(), NB, (int)nblk, (int)n, p->off.as<int64_t>(), d_counts);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_total.e1, s));
    p->t_check.timed = p->t_total.timed = true, p->t_unique.timed = p->ran_unique = unique != 0;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

// Device time of the last run: the check kernel, the duplicate kernel (0 when the run had unique = 0) and the whole call with the counts.
int pcs_fuse_last_kernel_ms(pcs_depth_fuser *p, float *check_ms, float *unique_ms, float *total_ms) {
    const char *who = "pcs_fuse_last_kernel_ms";
    if (!p || !check_ms || !unique_ms || !total_ms) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (const int rc = timer_ms(who, &p->t_check, check_ms, "nothing has run yet")) return rc;
    *unique_ms = 0.0f;
    if (p->ran_unique)
        if (const int rc = timer_ms(who, &p->t_unique, unique_ms, "nothing has run yet")) return rc;
    return timer_ms(who, &p->t_total, total_ms, "nothing has run yet");
}

}  // extern "C"
