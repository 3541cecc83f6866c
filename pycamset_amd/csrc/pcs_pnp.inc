// pcs_pnp.inc — host side of the batched target-pose estimation (included by pcs_engine.hip; kernels: ba_pnp.hpp).
extern "C" {
// ---- batched PnP (SURVEY f5): a handle that owns the camera table, the template, the observation copies and the outputs, in the
// style of pcs_triangulator.
struct pcs_pose_estimator {
    int device = 0;
    int64_t n_cams = 0, n_keys = 0;
    bool have_cams = false, have_template = false;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, done = nullptr;
    hipStream_t done_stream = nullptr;
    bool timed = false, have_done = false;
    double *d_tab = nullptr, *d_pts = nullptr;
    // handle-owned copies of the observations (grown on demand)
    int32_t *d_key = nullptr, *d_vcam = nullptr; double *d_uv = nullptr; int64_t *d_start = nullptr;
    int64_t key_capacity = 0, uv_capacity = 0, start_capacity = 0, vcam_capacity = 0;
    int64_t n_obs = 0, n_views = -1;
    int32_t *d_order = nullptr, *d_hist = nullptr;   // views by observation count (tri_order_*_kernel), built by the first run of a set of observations
    int64_t order_capacity = 0;
    bool order_valid = false;
    // handle-owned outputs
    double *d_pose = nullptr, *d_init = nullptr, *d_alt = nullptr, *d_rms = nullptr, *d_res = nullptr; int32_t *d_info = nullptr;
    int64_t pose_capacity = 0, init_capacity = 0, alt_capacity = 0, rms_capacity = 0, res_capacity = 0, info_capacity = 0;
    int owned = 0;            // PCS_PNP_OUT_* bits: which outputs of the last run are handle-owned
    bool run_valid = false;   // a run since the cameras / template / observations were last set
};

static hipError_t pnp_wait_done_host(pcs_pose_estimator *p) { return p->have_done ? hipEventSynchronize(p->done) : hipSuccess; }

int pcs_pnp_create(pcs_pose_estimator **out, int device, int64_t n_cams, int64_t n_keys) {
    if (!out || n_cams <= 0 || n_keys <= 0 || n_cams > INT32_MAX || n_keys > INT32_MAX) return fail(PCS_ERR_ARG, "pcs_pnp_create: bad arguments");
    *out = nullptr;
    const int ndev = pcs_device_count();
    if (ndev <= 0) return fail(PCS_ERR_NODEVICE, "pcs_pnp_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(PCS_ERR_ARG, "pcs_pnp_create: device out of range");
    HIPCHK(hipSetDevice(device));
    pcs_pose_estimator *p = new pcs_pose_estimator();
    p->device = device;
    p->n_cams = n_cams;
    p->n_keys = n_keys;
    hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&p->e0);
    if (e == hipSuccess) e = hipEventCreate(&p->e1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&p->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&p->d_tab, sizeof(double) * n_cams * TRI_CAM_STRIDE);
    if (e == hipSuccess) e = hipMalloc(&p->d_pts, sizeof(double) * n_keys * 3);
    if (e == hipSuccess) e = hipMalloc(&p->d_hist, sizeof(int32_t) * 512);
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_pnp_create: %s", hipGetErrorString(e));
        pcs_pnp_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_pnp_destroy(pcs_pose_estimator *p) {
    if (!p) return PCS_OK;
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    (void)pnp_wait_done_host(p);   // a run on a caller stream may still read the tables
    for (void *b : {(void *)p->d_tab, (void *)p->d_pts, (void *)p->d_key, (void *)p->d_vcam, (void *)p->d_uv, (void *)p->d_start, (void *)p->d_order,
                    (void *)p->d_hist, (void *)p->d_pose, (void *)p->d_init, (void *)p->d_alt, (void *)p->d_rms, (void *)p->d_res, (void *)p->d_info})
        if (b) (void)hipFree(b);
    if (p->e0) (void)hipEventDestroy(p->e0);
    if (p->e1) (void)hipEventDestroy(p->e1);
    if (p->done) (void)hipEventDestroy(p->done);
    if (p->stream) (void)hipStreamDestroy(p->stream);
    delete p;
    return PCS_OK;
}

int pcs_pnp_set_cameras(pcs_pose_estimator *p, const double *intr) {
    if (!p || !intr) return fail(PCS_ERR_ARG, "pcs_pnp_set_cameras: bad arguments");
    std::vector<double> tab((size_t)p->n_cams * TRI_CAM_STRIDE, 0.0);
    for (int64_t c = 0; c < p->n_cams; ++c)
        for (int k = 0; k < 9; ++k) tab[c * TRI_CAM_STRIDE + 22 + k] = intr[9 * c + k];   // [fx cx fy cy k0 k1 p0 p1 k2]: the slab row as it is
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(pnp_wait_done_host(p));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(p->d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    p->have_cams = true;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_pnp_set_template(pcs_pose_estimator *p, const double *points) {
    if (!p || !points) return fail(PCS_ERR_ARG, "pcs_pnp_set_template: bad arguments");
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(pnp_wait_done_host(p));
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipMemcpy(p->d_pts, points, sizeof(double) * 3 * p->n_keys, hipMemcpyHostToDevice));
    p->have_template = true;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_pnp_set_observations(pcs_pose_estimator *p, int64_t n_obs, const int32_t *key, const double *uv, int64_t n_views, const int64_t *start_inds,
                             const int32_t *view_cam) {
    if (!p || n_obs < 0 || n_views < 0 || n_views > INT32_MAX || !start_inds || (n_obs > 0 && (!key || !uv)) || (n_views > 0 && !view_cam))
        return fail(PCS_ERR_ARG, "pcs_pnp_set_observations: bad arguments");
    if (start_inds[0] != 0 || start_inds[n_views] != n_obs) return fail(PCS_ERR_ARG, "pcs_pnp_set_observations: start_inds must run from 0 to n_obs");
    for (int64_t j = 0; j < n_views; ++j) {
        if (start_inds[j + 1] < start_inds[j]) return fail(PCS_ERR_ARG, "pcs_pnp_set_observations: start_inds must be non-decreasing");
        if (view_cam[j] < 0 || view_cam[j] >= p->n_cams)
            return fail(PCS_ERR_RANGE, "view %lld has camera %d outside [0,%lld)", (long long)j, view_cam[j], (long long)p->n_cams);
    }
    for (int64_t r = 0; r < n_obs; ++r)
        if (key[r] < 0 || key[r] >= p->n_keys) return fail(PCS_ERR_RANGE, "observation %lld has key %d outside [0,%lld)", (long long)r, key[r], (long long)p->n_keys);
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(pnp_wait_done_host(p));   // a run queued on ANY stream may still read the observation copies
    HIPCHK(hipStreamSynchronize(p->stream));
    p->n_views = -1;
    int rc;
    if ((rc = tri_grow((void **)&p->d_key, &p->key_capacity, std::max<int64_t>(1, n_obs), sizeof(int32_t)))) return rc;
    if ((rc = tri_grow((void **)&p->d_uv, &p->uv_capacity, std::max<int64_t>(1, n_obs), 2 * sizeof(double)))) return rc;
    if ((rc = tri_grow((void **)&p->d_start, &p->start_capacity, n_views + 1, sizeof(int64_t)))) return rc;
    if ((rc = tri_grow((void **)&p->d_vcam, &p->vcam_capacity, std::max<int64_t>(1, n_views), sizeof(int32_t)))) return rc;
    if (n_obs) {
        HIPCHK(hipMemcpyAsync(p->d_key, key, sizeof(int32_t) * n_obs, hipMemcpyHostToDevice, p->stream));
        HIPCHK(hipMemcpyAsync(p->d_uv, uv, sizeof(double) * 2 * n_obs, hipMemcpyHostToDevice, p->stream));
    }
    if (n_views) HIPCHK(hipMemcpyAsync(p->d_vcam, view_cam, sizeof(int32_t) * n_views, hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipMemcpyAsync(p->d_start, start_inds, sizeof(int64_t) * (n_views + 1), hipMemcpyHostToDevice, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));   // the caller may reuse its host arrays
    p->n_obs = n_obs;
    p->n_views = n_views;
    p->order_valid = false;
    p->run_valid = false;
    return PCS_OK;
}

static_assert(PNP_NOT_ESTIMATED == PCS_PNP_NOT_ESTIMATED && PNP_CONVERGED == PCS_PNP_CONVERGED && PNP_MAX_ITER == PCS_PNP_MAX_ITER &&
              PNP_NO_DECREASE == PCS_PNP_NO_DECREASE, "status codes of pcs_hip.h");
// lanes per view, observations held in registers per lane (profiles/r10: kernel resources; no times measured yet)
constexpr int PNP_G = 16, PNP_V = 4;

int pcs_pnp_run(pcs_pose_estimator *p, int max_iter, double ftol, double xtol, double gtol, int min_points, int flags, double *d_pose,
                double *d_pose_init, double *d_pose_alt, double *d_rms, int32_t *d_info, double *d_resid, void *stream) {
    if (max_iter < 0 || !(ftol >= 0.0 && ftol < INFINITY) || !(xtol >= 0.0 && xtol < INFINITY) || !(gtol >= 0.0 && gtol < INFINITY) || min_points < 1 ||
        (flags & ~PCS_PNP_RESIDUALS))
        return fail(PCS_ERR_ARG, "pcs_pnp_run: bad options (max_iter >= 0, finite tolerances >= 0, min_points >= 1, flags PCS_PNP_RESIDUALS)");
    if (!p) return fail(PCS_ERR_ARG, "pcs_pnp_run: NULL handle");
    if (!p->have_cams || !p->have_template || p->n_views < 0) return fail(PCS_ERR_STATE, "pcs_pnp_run: cameras, template or observations not set");
    const bool want_resid = flags & PCS_PNP_RESIDUALS;
    const int owned = (d_pose ? 0 : PCS_PNP_OUT_POSE) | (d_pose_init ? 0 : PCS_PNP_OUT_POSE_INIT) | (d_pose_alt ? 0 : PCS_PNP_OUT_POSE_ALT) |
                      (d_rms ? 0 : PCS_PNP_OUT_RMS) | (d_info ? 0 : PCS_PNP_OUT_INFO) | (want_resid && !d_resid ? PCS_PNP_OUT_RESIDUALS : 0);
    if (p->n_views == 0) {
        p->owned = owned;
        p->run_valid = true;
        p->timed = false;   // nothing ran: no time of an earlier run is reported for this one
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(p->device));
    hipStream_t s = stream ? (hipStream_t)stream : p->stream;
    const int64_t nv = p->n_views;
    const bool grows = ((owned & PCS_PNP_OUT_POSE) && nv > p->pose_capacity) || ((owned & PCS_PNP_OUT_POSE_INIT) && nv > p->init_capacity) ||
                       ((owned & PCS_PNP_OUT_POSE_ALT) && nv > p->alt_capacity) || ((owned & PCS_PNP_OUT_RMS) && nv > p->rms_capacity) ||
                       ((owned & PCS_PNP_OUT_INFO) && nv > p->info_capacity) || ((owned & PCS_PNP_OUT_RESIDUALS) && p->n_obs > p->res_capacity) ||
                       (!p->order_valid && nv > p->order_capacity);
    if (p->have_done) {   // outputs and the order are shared between runs: the previous one finishes first
        if (grows || s == hipStreamLegacy || p->done_stream == hipStreamLegacy) HIPCHK(hipEventSynchronize(p->done));   // frees need the host to wait
        else if (s != p->done_stream) HIPCHK(hipStreamWaitEvent(s, p->done, 0));
    }
    int rc;
    if (owned & PCS_PNP_OUT_POSE) { if ((rc = tri_grow((void **)&p->d_pose, &p->pose_capacity, nv, 6 * sizeof(double)))) return rc; d_pose = p->d_pose; }
    if (owned & PCS_PNP_OUT_POSE_INIT) { if ((rc = tri_grow((void **)&p->d_init, &p->init_capacity, nv, 6 * sizeof(double)))) return rc; d_pose_init = p->d_init; }
    if (owned & PCS_PNP_OUT_POSE_ALT) { if ((rc = tri_grow((void **)&p->d_alt, &p->alt_capacity, nv, 6 * sizeof(double)))) return rc; d_pose_alt = p->d_alt; }
    if (owned & PCS_PNP_OUT_RMS) { if ((rc = tri_grow((void **)&p->d_rms, &p->rms_capacity, nv, 2 * sizeof(double)))) return rc; d_rms = p->d_rms; }
    if (owned & PCS_PNP_OUT_INFO) { if ((rc = tri_grow((void **)&p->d_info, &p->info_capacity, nv, 3 * sizeof(int32_t)))) return rc; d_info = p->d_info; }
    if (owned & PCS_PNP_OUT_RESIDUALS) {
        if ((rc = tri_grow((void **)&p->d_res, &p->res_capacity, std::max<int64_t>(1, p->n_obs), 2 * sizeof(double)))) return rc;
        d_resid = p->d_res;
    }
    if (!p->order_valid && (rc = tri_grow((void **)&p->d_order, &p->order_capacity, nv, sizeof(int32_t)))) return rc;
    HIPCHK(hipEventRecord(p->e0, s));   // after every allocation: nothing is queued by a call that fails in one
    if (!p->order_valid) {   // views of like size side by side: a wave does not mix 6-point and 486-point views (counts above 255 share a bucket)
        HIPCHK(hipMemsetAsync(p->d_hist, 0, sizeof(int32_t) * 512, s));
        const dim3 pg((unsigned)((nv + 255) / 256));
        hipLaunchKernelGGL(tri_order_count_kernel, pg, dim3(256), 0, s, (const int64_t *)p->d_start, nv, p->d_hist);
        hipLaunchKernelGGL(tri_order_scan_kernel, dim3(1), dim3(256), 0, s, p->d_hist);
        hipLaunchKernelGGL(tri_order_scatter_kernel, pg, dim3(256), 0, s, (const int64_t *)p->d_start, nv, p->d_hist, p->d_order);
        HIPCHK(hipGetLastError());
        p->order_valid = true;
    }
    const dim3 grid((unsigned)((nv * PNP_G + 255) / 256));
    hipLaunchKernelGGL((pnp_start_kernel<PNP_G>), grid, dim3(256), 0, s, (const int32_t *)p->d_key, (const double2 *)p->d_uv, (const int64_t *)p->d_start,
                       (const int32_t *)p->d_vcam, (const double *)p->d_tab, (const double *)p->d_pts, nv, (const int32_t *)p->d_order, min_points,
                       d_pose_init, d_pose_alt);
    hipLaunchKernelGGL((pnp_lm_kernel<PNP_G, PNP_V>), grid, dim3(256), 0, s, (const int32_t *)p->d_key, (const double2 *)p->d_uv, (const int64_t *)p->d_start,
                       (const int32_t *)p->d_vcam, (const double *)p->d_tab, (const double *)p->d_pts, nv, (const int32_t *)p->d_order,
                       (const double *)d_pose_init, (const double *)d_pose_alt, max_iter, ftol, xtol, gtol, min_points, d_pose, d_rms, d_info,
                       want_resid ? d_resid : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->e1, s));
    p->timed = true;
    p->owned = owned;
    p->run_valid = true;
    p->have_done = true;
    p->done_stream = s;   // compared only, never used as a handle again
    HIPCHK(hipEventRecord(p->done, s));
    return PCS_OK;
}

int pcs_pnp_results(pcs_pose_estimator *p, double *pose, double *pose_init, double *pose_alt, double *rms, int32_t *info, double *resid) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_pnp_results: NULL handle");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_pnp_results: no run on the current cameras, template and observations (pcs_pnp_run first)");
    const int want = (pose ? PCS_PNP_OUT_POSE : 0) | (pose_init ? PCS_PNP_OUT_POSE_INIT : 0) | (pose_alt ? PCS_PNP_OUT_POSE_ALT : 0) |
                     (rms ? PCS_PNP_OUT_RMS : 0) | (info ? PCS_PNP_OUT_INFO : 0) | (resid ? PCS_PNP_OUT_RESIDUALS : 0);
    if (want & ~p->owned) return fail(PCS_ERR_STATE, "pcs_pnp_results: the last run wrote some of these outputs to caller buffers (or computed no residuals)");
    if (p->n_views == 0) return PCS_OK;
    HIPCHK(hipSetDevice(p->device));
    HIPCHK(pnp_wait_done_host(p));   // the run may have been queued on a caller stream
    const int64_t nv = p->n_views;
    if (pose) HIPCHK(hipMemcpyAsync(pose, p->d_pose, sizeof(double) * 6 * nv, hipMemcpyDeviceToHost, p->stream));
    if (pose_init) HIPCHK(hipMemcpyAsync(pose_init, p->d_init, sizeof(double) * 6 * nv, hipMemcpyDeviceToHost, p->stream));
    if (pose_alt) HIPCHK(hipMemcpyAsync(pose_alt, p->d_alt, sizeof(double) * 6 * nv, hipMemcpyDeviceToHost, p->stream));
    if (rms) HIPCHK(hipMemcpyAsync(rms, p->d_rms, sizeof(double) * 2 * nv, hipMemcpyDeviceToHost, p->stream));
    if (info) HIPCHK(hipMemcpyAsync(info, p->d_info, sizeof(int32_t) * 3 * nv, hipMemcpyDeviceToHost, p->stream));
    if (resid && p->n_obs) HIPCHK(hipMemcpyAsync(resid, p->d_res, sizeof(double) * 2 * p->n_obs, hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return PCS_OK;
}

int pcs_pnp_last_kernel_ms(pcs_pose_estimator *p, float *kernel_ms) {
    if (!p || !kernel_ms) return fail(PCS_ERR_ARG, "pcs_pnp_last_kernel_ms: bad arguments");
    if (!p->timed) return fail(PCS_ERR_STATE, "pcs_pnp_last_kernel_ms: nothing has run yet");
    HIPCHK(hipEventSynchronize(p->e1));
    HIPCHK(hipEventElapsedTime(kernel_ms, p->e0, p->e1));
    return PCS_OK;
}
}  // extern "C"
