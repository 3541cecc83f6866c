// pcs_triangulator.inc — host side of the batched triangulation (included by pcs_engine.hip; kernels: ba_triangulate.hpp, ba_tri_refine.hpp).
extern "C" {
// ---- batched triangulation (SURVEY f4): a handle that owns the camera table, the observation buffers and the
// kernel's scratch, so that repeated calls (CameraSet.multi_cam_triangulate per frame set, cameras/camera_set.py:343-402)
// pay neither allocations nor — with device-resident inputs — copies.
struct pcs_triangulator {
    int device = 0;
    int64_t n_cams = 0;
    bool have_cams = false;
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool timed = false;
    double *d_tab = nullptr;
    // handle-owned copies of host inputs (grown on demand)
    int32_t *d_cam = nullptr; double *d_uv = nullptr; int64_t *d_start = nullptr;
    int64_t obs_capacity = 0, uv_capacity = 0, pts_capacity = 0;
    // scratch + default output
    void *d_scr = nullptr, *d_scl = nullptr; double *d_pts = nullptr;
    int64_t scr_capacity = 0, scl_capacity = 0, out_capacity = 0;
    // current problem (device pointers: handle-owned or the caller's)
    const int32_t *cur_cam = nullptr; const double *cur_uv = nullptr; const int64_t *cur_start = nullptr;
    int64_t n_obs = 0, n_pts = -1;
    // the grouping in front of the triangulation (pcs_tri_group_device): per-feature counts, block sums of the scan, totals
    int32_t *d_count = nullptr; uint64_t *d_block_sums = nullptr; int64_t *d_totals = nullptr;
    int64_t count_capacity = 0, block_capacity = 0;
    int32_t *d_order = nullptr, *d_hist = nullptr;   // points by view count (built by the first run of a set of observations)
    int64_t order_capacity = 0;
    bool order_valid = false, sort_points = true;
    int variant = 1; // 1: views in registers + divide-free rotations (round 4; 3: eight instead of six register views per lane); 0: round 3's kernel (PCS_TRI_VARIANT=0)
    int lanes = 4;   // lanes per point: 1, 2, 4, 8 or 16 (profiles/r01/tri_legacy_bench.log: 4 is fastest at 2-22 views)
    // Ordering across streams, as in pcs_engine: `done` is recorded after every run; whatever touches the camera table, the
    // handle-owned observation copies, the scratch or the output next first waits for it — on the host where the host
    // writes or reads, with hipStreamWaitEvent where a run moves to another stream (scratch and output are shared).
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    bool have_done = false;
    bool out_owned = false;   // the last run wrote the handle-owned output (pcs_tri_points has something to return)
    // the refinement (pcs_tri_refine): it starts from the points of the last run on the current cameras and observations
    bool run_valid = false;          // a run since the cameras / observations were last set
    const double *run_pts = nullptr; // where that run wrote its points (handle-owned or the caller's buffer)
    double *d_rpts = nullptr, *d_rrms = nullptr, *d_rres = nullptr; int32_t *d_rinfo = nullptr;   // handle-owned refinement outputs
    int64_t rpts_capacity = 0, rrms_capacity = 0, rres_capacity = 0, rinfo_capacity = 0;
    int refine_owned = 0;            // PCS_TRI_OUT_* bits: which outputs of the last refinement are handle-owned
    bool refine_valid = false;       // a refinement since the last run (pcs_tri_refined has something to return)
    hipEvent_t r0 = nullptr, r1 = nullptr;
    bool refine_timed = false;
};

static hipError_t tri_wait_done_host(pcs_triangulator *t) { return t->have_done ? hipEventSynchronize(t->done) : hipSuccess; }

static int tri_grow(void **buf, int64_t *cap, int64_t need, size_t elem) {
    if (need <= *cap) return PCS_OK;
    if (*buf) HIPCHK(hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    HIPCHK(hipMalloc(buf, elem * (size_t)need));
    *cap = need;
    return PCS_OK;
}

int pcs_tri_create(pcs_triangulator **out, int device, int64_t n_cams) {
    if (!out || n_cams <= 0) return fail(PCS_ERR_ARG, "pcs_tri_create: bad arguments");
    *out = nullptr;
    const int ndev = pcs_device_count();
    if (ndev <= 0) return fail(PCS_ERR_NODEVICE, "pcs_tri_create: no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(PCS_ERR_ARG, "pcs_tri_create: device out of range");
    HIPCHK(hipSetDevice(device));
    pcs_triangulator *t = new pcs_triangulator();
    t->device = device;
    t->n_cams = n_cams;
    const char *lanes_env = getenv("PCS_TRI_LANES");   // A/B switch
    const int lanes = lanes_env ? atoi(lanes_env) : 4;
    t->lanes = (lanes == 1 || lanes == 2 || lanes == 8 || lanes == 16) ? lanes : 4;
    const char *var_env = getenv("PCS_TRI_VARIANT");
    t->variant = var_env ? atoi(var_env) : 1;
    t->sort_points = getenv("PCS_TRI_NO_SORT") == nullptr;   // A/B switch
    hipError_t e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&t->e0);
    if (e == hipSuccess) e = hipEventCreate(&t->e1);
    if (e == hipSuccess) e = hipEventCreate(&t->r0);
    if (e == hipSuccess) e = hipEventCreate(&t->r1);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&t->done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc(&t->d_tab, sizeof(double) * n_cams * TRI_CAM_STRIDE);
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_tri_create: %s", hipGetErrorString(e));
        pcs_tri_destroy(t);
        return rc;
    }
    *out = t;
    return PCS_OK;
}

int pcs_tri_destroy(pcs_triangulator *t) {
    if (!t) return PCS_OK;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    (void)tri_wait_done_host(t);   // a run on a caller stream may still read the tables
    for (void *b : {(void *)t->d_tab, (void *)t->d_cam, (void *)t->d_uv, (void *)t->d_start, t->d_scr, t->d_scl, (void *)t->d_pts, (void *)t->d_order, (void *)t->d_hist,
                    (void *)t->d_count, (void *)t->d_block_sums, (void *)t->d_totals, (void *)t->d_rpts, (void *)t->d_rrms, (void *)t->d_rres,
                    (void *)t->d_rinfo})
        if (b) (void)hipFree(b);
    if (t->e0) (void)hipEventDestroy(t->e0);
    if (t->e1) (void)hipEventDestroy(t->e1);
    if (t->r0) (void)hipEventDestroy(t->r0);
    if (t->r1) (void)hipEventDestroy(t->r1);
    if (t->done) (void)hipEventDestroy(t->done);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
    return PCS_OK;
}

int pcs_tri_set_cameras(pcs_triangulator *t, const double *proj, const double *intrinsics, const double *dists) {
    if (!t || !proj || !intrinsics || !dists) return fail(PCS_ERR_ARG, "pcs_tri_set_cameras: bad arguments");
    std::vector<double> tab((size_t)t->n_cams * TRI_CAM_STRIDE, 0.0);
    for (int64_t c = 0; c < t->n_cams; ++c) {
        double *r = tab.data() + c * TRI_CAM_STRIDE;
        for (int k = 0; k < 12; ++k) r[k] = proj[12 * c + k];
        const double *K = intrinsics + 9 * c;
        r[22] = K[0]; r[23] = K[2]; r[24] = K[4]; r[25] = K[5];
        for (int k = 0; k < 5; ++k) r[26 + k] = dists[5 * c + k];
    }
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(tri_wait_done_host(t));   // a run queued on ANY stream may still read the table
    HIPCHK(hipStreamSynchronize(t->stream));
    HIPCHK(hipMemcpy(t->d_tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    t->have_cams = true;
    t->run_valid = t->refine_valid = false;   // a refinement must start from points of these cameras
    return PCS_OK;
}

int pcs_tri_set_observations(pcs_triangulator *t, int64_t n_obs, const int32_t *cam, const double *uv, int64_t n_pts, const int64_t *start_inds) {
    if (!t || n_obs < 0 || n_pts < 0 || !start_inds || (n_obs > 0 && (!cam || !uv))) return fail(PCS_ERR_ARG, "pcs_tri_set_observations: bad arguments");
    if (start_inds[0] != 0 || start_inds[n_pts] != n_obs) return fail(PCS_ERR_ARG, "pcs_tri_set_observations: start_inds must run from 0 to n_obs");
    for (int64_t j = 0; j < n_pts; ++j)
        if (start_inds[j + 1] < start_inds[j]) return fail(PCS_ERR_ARG, "pcs_tri_set_observations: start_inds must be non-decreasing");
    for (int64_t r = 0; r < n_obs; ++r)
        if (cam[r] < 0 || cam[r] >= t->n_cams) return fail(PCS_ERR_RANGE, "observation %lld has camera %d outside [0,%lld)", (long long)r, cam[r], (long long)t->n_cams);
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(tri_wait_done_host(t));   // a run queued on ANY stream may still read the observation copies
    HIPCHK(hipStreamSynchronize(t->stream));
    t->n_pts = -1;
    int rc = tri_grow((void **)&t->d_cam, &t->obs_capacity, std::max<int64_t>(1, n_obs), sizeof(int32_t));
    if (rc) return rc;
    rc = tri_grow((void **)&t->d_uv, &t->uv_capacity, std::max<int64_t>(1, n_obs), 2 * sizeof(double));
    if (rc) return rc;
    rc = tri_grow((void **)&t->d_start, &t->pts_capacity, n_pts + 1, sizeof(int64_t));
    if (rc) return rc;
    if (n_obs) {
        HIPCHK(hipMemcpyAsync(t->d_cam, cam, sizeof(int32_t) * n_obs, hipMemcpyHostToDevice, t->stream));
        HIPCHK(hipMemcpyAsync(t->d_uv, uv, sizeof(double) * 2 * n_obs, hipMemcpyHostToDevice, t->stream));
    }
    HIPCHK(hipMemcpyAsync(t->d_start, start_inds, sizeof(int64_t) * (n_pts + 1), hipMemcpyHostToDevice, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));   // the caller may reuse its host arrays
    t->cur_cam = t->d_cam; t->cur_uv = t->d_uv; t->cur_start = t->d_start;
    t->n_obs = n_obs; t->n_pts = n_pts;
    t->order_valid = false;
    t->out_owned = false;   // results of an earlier problem are not this problem's
    t->run_valid = t->refine_valid = false;
    return PCS_OK;
}

int pcs_tri_set_observations_device(pcs_triangulator *t, int64_t n_obs, const int32_t *d_cam, const double *d_uv, int64_t n_pts, const int64_t *d_start_inds) {
    if (!t || n_obs < 0 || n_pts < 0 || !d_start_inds || (n_obs > 0 && (!d_cam || !d_uv))) return fail(PCS_ERR_ARG, "pcs_tri_set_observations_device: bad arguments");
    t->cur_cam = d_cam; t->cur_uv = d_uv; t->cur_start = d_start_inds;   // caller-owned, not range-checked (stay on the device)
    t->n_obs = n_obs; t->n_pts = n_pts;
    t->order_valid = false;
    t->out_owned = false;
    t->run_valid = t->refine_valid = false;
    return PCS_OK;
}

// The grouping CameraSet.multi_cam_triangulate does in front of nb_triangulate_full (cameras/camera_set.py:371-378), on the device
// (csrc/ba_triangulate.hpp, "the grouping in front of the triangulation"): from n table rows (camera, dense feature id, measurement;
// caller-owned device arrays, the table grouped by feature) to the handle's current observations — the rows of features seen by at
// least two cameras, in table order, and their start indices.  One host synchronisation (the counts).  *grouped = 0: the table is
// NOT grouped by feature (a feature's rows are not consecutive): nothing was set, the caller groups on the host.
int pcs_tri_group_device(pcs_triangulator *t, int64_t n, const int32_t *d_cam, const int32_t *d_feat, const double *d_uv, int64_t n_features,
                         int64_t *n_pts, int64_t *n_kept, int32_t *grouped, void *stream) {
    if (!t || n < 0 || n > INT32_MAX || n_features <= 0 || n_features > INT32_MAX || !n_pts || !n_kept || !grouped || (n > 0 && (!d_cam || !d_feat || !d_uv)))
        return fail(PCS_ERR_ARG, "pcs_tri_group_device: bad arguments");
    *n_pts = *n_kept = 0;
    *grouped = 1;
    HIPCHK(hipSetDevice(t->device));
    hipStream_t s = stream ? (hipStream_t)stream : t->stream;
    HIPCHK(tri_wait_done_host(t));   // a run queued on ANY stream may still read the observation copies this call overwrites
    HIPCHK(hipStreamSynchronize(t->stream));
    t->n_pts = -1;
    t->run_valid = t->refine_valid = false;
    if (n == 0) {
        int rc0 = tri_grow((void **)&t->d_start, &t->pts_capacity, 1, sizeof(int64_t));
        if (rc0) return rc0;
        HIPCHK(hipMemsetAsync(t->d_start, 0, sizeof(int64_t), s));
        HIPCHK(hipStreamSynchronize(s));
        t->cur_cam = t->d_cam; t->cur_uv = t->d_uv; t->cur_start = t->d_start;
        t->n_obs = 0; t->n_pts = 0; t->order_valid = false; t->out_owned = false;
        return PCS_OK;
    }
    const int64_t n_blocks = (n + TRI_GROUP_BLOCK - 1) / TRI_GROUP_BLOCK;
    int rc = tri_grow((void **)&t->d_cam, &t->obs_capacity, n, sizeof(int32_t));
    if (rc) return rc;
    rc = tri_grow((void **)&t->d_uv, &t->uv_capacity, n, 2 * sizeof(double));
    if (rc) return rc;
    // one entry per kept run + 1.  A GROUPED table has at most n / 2 kept runs, but whether it is grouped is only known afterwards: in a table
    // whose features interleave every row can be the head of a kept run (writes up to start[n]; sized for n / 2 + 2 until this was found
    // by a fault in the full test suite — alone, the overrun stayed inside the allocation)
    rc = tri_grow((void **)&t->d_start, &t->pts_capacity, n + 2, sizeof(int64_t));
    if (rc) return rc;
    rc = tri_grow((void **)&t->d_count, &t->count_capacity, n_features, sizeof(int32_t));
    if (rc) return rc;
    rc = tri_grow((void **)&t->d_block_sums, &t->block_capacity, n_blocks, sizeof(uint64_t));
    if (rc) return rc;
    if (!t->d_totals) HIPCHK(hipMalloc(&t->d_totals, sizeof(int64_t) * 4));
    HIPCHK(hipMemsetAsync(t->d_count, 0, sizeof(int32_t) * n_features, s));
    HIPCHK(hipMemsetAsync(t->d_totals, 0, sizeof(int64_t) * 4, s));
    TriGroupArgs a{d_cam, d_feat, reinterpret_cast<const double2 *>(d_uv), t->d_count, t->d_block_sums, t->d_totals, t->d_cam,
                   reinterpret_cast<double2 *>(t->d_uv), t->d_start, n, n_features, (int32_t)n_blocks};
    hipLaunchKernelGGL(tri_group_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tri_group_blocksum_kernel, dim3((unsigned)n_blocks), dim3(TRI_GROUP_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tri_group_scan_sums_kernel, dim3(1), dim3(TRI_GROUP_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tri_group_scatter_kernel, dim3((unsigned)n_blocks), dim3(TRI_GROUP_BLOCK), 0, s, a);
    HIPCHK(hipGetLastError());
    int64_t totals[4];
    HIPCHK(hipMemcpyAsync(totals, t->d_totals, sizeof totals, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (totals[2] != totals[3]) {   // more runs than features: some feature's rows are not consecutive
        *grouped = 0;
        return PCS_OK;
    }
    *n_kept = totals[0];
    *n_pts = totals[1];
    t->cur_cam = t->d_cam; t->cur_uv = t->d_uv; t->cur_start = t->d_start;
    t->n_obs = totals[0]; t->n_pts = totals[1];
    t->order_valid = false;
    t->out_owned = false;
    return PCS_OK;
}

int pcs_tri_run(pcs_triangulator *t, double *d_pts, void *stream) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_run: bad arguments");
    if (!t->have_cams) return fail(PCS_ERR_STATE, "pcs_tri_run: cameras not set");
    if (t->n_pts < 0) return fail(PCS_ERR_STATE, "pcs_tri_run: observations not set");
    t->refine_valid = false;
    if (t->n_pts == 0) {
        t->run_valid = true;
        t->run_pts = d_pts;
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(t->device));
    hipStream_t s = stream ? (hipStream_t)stream : t->stream;
    const bool need_order = t->variant != 0 && t->sort_points && !t->order_valid && t->n_pts < (1ll << 31);
    const bool grows = t->n_obs > t->scr_capacity || t->n_obs > t->scl_capacity || (!d_pts && t->n_pts > t->out_capacity) || (need_order && t->n_pts > t->order_capacity);
    if (t->have_done) {   // scratch and output are shared between runs: the previous one finishes first
        if (grows || s == hipStreamLegacy || t->done_stream == hipStreamLegacy) HIPCHK(hipEventSynchronize(t->done));   // frees need the host to wait
        else if (s != t->done_stream) HIPCHK(hipStreamWaitEvent(s, t->done, 0));
    }
    int rc = tri_grow(&t->d_scr, &t->scr_capacity, std::max<int64_t>(1, t->n_obs), 4 * sizeof(double));   // Householder row r_i per observation
    if (rc) return rc;
    rc = tri_grow(&t->d_scl, &t->scl_capacity, std::max<int64_t>(1, t->n_obs), 2 * sizeof(double));   // (1 / E_i, lambda_i)
    if (rc) return rc;
    const bool owned = !d_pts;
    if (owned) {
        rc = tri_grow((void **)&t->d_pts, &t->out_capacity, t->n_pts, 3 * sizeof(double));
        if (rc) return rc;
        d_pts = t->d_pts;
    }
    const int lanes = t->lanes;
    const dim3 grid((unsigned)((t->n_pts * lanes + 255) / 256));
    if (need_order) {
        // the visiting order of this set of observations, on the run's own stream (the caller's start_inds may have been produced there)
        rc = tri_grow((void **)&t->d_order, &t->order_capacity, t->n_pts, sizeof(int32_t));
        if (rc) return rc;
        if (!t->d_hist) HIPCHK(hipMalloc(&t->d_hist, sizeof(int32_t) * 512));
        HIPCHK(hipMemsetAsync(t->d_hist, 0, sizeof(int32_t) * 512, s));
        const dim3 pg((unsigned)((t->n_pts + 255) / 256));
        hipLaunchKernelGGL(tri_order_count_kernel, pg, dim3(256), 0, s, t->cur_start, t->n_pts, t->d_hist);
        hipLaunchKernelGGL(tri_order_scan_kernel, dim3(1), dim3(256), 0, s, t->d_hist);
        hipLaunchKernelGGL(tri_order_scatter_kernel, pg, dim3(256), 0, s, t->cur_start, t->n_pts, t->d_hist, t->d_order);
        HIPCHK(hipGetLastError());
        t->order_valid = true;
    }
#define PCS_TRI_LAUNCH(G_)                                                                                                     \
    hipExtLaunchKernelGGL(triangulate_kernel<G_>, grid, dim3(256), 0, s, t->e0, t->e1, 0, t->cur_cam, (const double2 *)t->cur_uv, \
                          t->cur_start, (const double *)t->d_tab, (double4 *)t->d_scr, (double2 *)t->d_scl, d_pts, t->n_pts)
#define PCS_TRI_LAUNCH_REG(G_, V_)                                                                                                     \
    hipExtLaunchKernelGGL((triangulate_reg_kernel<G_, V_>), grid, dim3(256), 0, s, t->e0, t->e1, 0, t->cur_cam, (const double2 *)t->cur_uv, \
                          t->cur_start, (const double *)t->d_tab, (double4 *)t->d_scr, (double2 *)t->d_scl, d_pts, t->n_pts, (const int32_t *)(t->order_valid ? t->d_order : nullptr))
    if (t->variant == 0) {   // round 3's form (views in the global scratch, IEEE divides): kept for A/B (PCS_TRI_VARIANT=0)
        if (lanes == 1) PCS_TRI_LAUNCH(1);
        else if (lanes == 2) PCS_TRI_LAUNCH(2);
        else if (lanes == 8) PCS_TRI_LAUNCH(8);
        else if (lanes == 16) PCS_TRI_LAUNCH(16);
        else PCS_TRI_LAUNCH(4);
    } else {                 // views in registers (6 or 8 per lane; further ones in the scratch), divide-free rotations
        if (lanes == 1) PCS_TRI_LAUNCH_REG(1, 8);
        else if (lanes == 2) PCS_TRI_LAUNCH_REG(2, 8);
        else if (lanes == 8) PCS_TRI_LAUNCH_REG(8, 8);
        else if (lanes == 16) PCS_TRI_LAUNCH_REG(16, 8);
        else if (t->variant == 3) PCS_TRI_LAUNCH_REG(4, 8);
        else PCS_TRI_LAUNCH_REG(4, 6);   // 24 views in registers at 156 VGPRs (three waves per SIMD): 47 us against 52 us for (4, 8); (4, 3) — four waves
                                         // per SIMD, 12 register views, the rest through the scratch records — 53 us, (4, 4) 49 us (profiles/r05/tri_bench_r05.log)
    }
#undef PCS_TRI_LAUNCH_REG
#undef PCS_TRI_LAUNCH
    HIPCHK(hipGetLastError());
    t->timed = true;
    t->out_owned = owned;
    t->run_valid = true;
    t->run_pts = d_pts;
    t->have_done = true;
    t->done_stream = s;   // compared only, never used as a handle again
    HIPCHK(hipEventRecord(t->done, s));
    return PCS_OK;
}

// The refinement of the last run's points (csrc/ba_tri_refine.hpp): per-point LM on the reprojection error in the measured pixels.
static_assert(TRI_REFINE_NOT_REFINED == PCS_TRI_REFINE_NOT_REFINED && TRI_REFINE_CONVERGED == PCS_TRI_REFINE_CONVERGED &&
              TRI_REFINE_MAX_ITER == PCS_TRI_REFINE_MAX_ITER && TRI_REFINE_NO_DECREASE == PCS_TRI_REFINE_NO_DECREASE, "status codes of pcs_hip.h");
int pcs_tri_refine(pcs_triangulator *t, int max_iter, double ftol, double xtol, double gtol, int flags, double *d_pts, double *d_rms,
                   int32_t *d_info, double *d_resid, void *stream) {
    if (max_iter < 0 || !(ftol >= 0.0 && ftol < INFINITY) || !(xtol >= 0.0 && xtol < INFINITY) || !(gtol >= 0.0 && gtol < INFINITY) ||
        (flags & ~PCS_TRI_REFINE_RESIDUALS))
        return fail(PCS_ERR_ARG, "pcs_tri_refine: bad options (max_iter >= 0, finite tolerances >= 0, flags PCS_TRI_REFINE_RESIDUALS)");
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_refine: NULL handle");
    if (!t->have_cams || t->n_pts < 0 || !t->run_valid)
        return fail(PCS_ERR_STATE, "pcs_tri_refine: no run on the current cameras and observations (pcs_tri_run first)");
    const bool want_resid = flags & PCS_TRI_REFINE_RESIDUALS;
    const int owned = (d_pts ? 0 : PCS_TRI_OUT_POINTS) | (d_rms ? 0 : PCS_TRI_OUT_RMS) | (d_info ? 0 : PCS_TRI_OUT_INFO) |
                      (want_resid && !d_resid ? PCS_TRI_OUT_RESIDUALS : 0);
    if (t->n_pts == 0) {
        t->refine_owned = owned;
        t->refine_valid = true;
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(t->device));
    hipStream_t s = stream ? (hipStream_t)stream : t->stream;
    const bool grows = ((owned & PCS_TRI_OUT_POINTS) && t->n_pts > t->rpts_capacity) || ((owned & PCS_TRI_OUT_RMS) && t->n_pts > t->rrms_capacity) ||
                       ((owned & PCS_TRI_OUT_INFO) && t->n_pts > t->rinfo_capacity) || ((owned & PCS_TRI_OUT_RESIDUALS) && t->n_obs > t->rres_capacity);
    if (t->have_done) {   // the run (or an earlier refinement) first: this reads its points and shares the outputs
        if (grows || s == hipStreamLegacy || t->done_stream == hipStreamLegacy) HIPCHK(hipEventSynchronize(t->done));
        else if (s != t->done_stream) HIPCHK(hipStreamWaitEvent(s, t->done, 0));
    }
    int rc;
    if (owned & PCS_TRI_OUT_POINTS) {
        if ((rc = tri_grow((void **)&t->d_rpts, &t->rpts_capacity, t->n_pts, 3 * sizeof(double)))) return rc;
        d_pts = t->d_rpts;
    }
    if (owned & PCS_TRI_OUT_RMS) {
        if ((rc = tri_grow((void **)&t->d_rrms, &t->rrms_capacity, t->n_pts, 2 * sizeof(double)))) return rc;
        d_rms = t->d_rrms;
    }
    if (owned & PCS_TRI_OUT_INFO) {
        if ((rc = tri_grow((void **)&t->d_rinfo, &t->rinfo_capacity, t->n_pts, 3 * sizeof(int32_t)))) return rc;
        d_info = t->d_rinfo;
    }
    if (owned & PCS_TRI_OUT_RESIDUALS) {
        if ((rc = tri_grow((void **)&t->d_rres, &t->rres_capacity, std::max<int64_t>(1, t->n_obs), 2 * sizeof(double)))) return rc;
        d_resid = t->d_rres;
    }
    constexpr int G = 4, V = 6;   // the DLT kernel's default geometry (profiles/r09: resources and time)
    const dim3 grid((unsigned)((t->n_pts * G + 255) / 256));
    hipExtLaunchKernelGGL((triangulate_refine_kernel<G, V>), grid, dim3(256), 0, s, t->r0, t->r1, 0, t->cur_cam, (const double2 *)t->cur_uv,
                          t->cur_start, (const double *)t->d_tab, t->run_pts, t->n_pts, (const int32_t *)(t->order_valid ? t->d_order : nullptr),
                          max_iter, ftol, xtol, gtol, d_pts, d_rms, d_info, want_resid ? d_resid : nullptr);
    HIPCHK(hipGetLastError());
    t->refine_timed = true;
    t->refine_owned = owned;
    t->refine_valid = true;
    t->have_done = true;
    t->done_stream = s;
    HIPCHK(hipEventRecord(t->done, s));
    return PCS_OK;
}

int pcs_tri_refined(pcs_triangulator *t, double *pts, double *rms, int32_t *info, double *resid) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_refined: NULL handle");
    if (!t->refine_valid) return fail(PCS_ERR_STATE, "pcs_tri_refined: no refinement since the last run (pcs_tri_refine first)");
    const int want = (pts ? PCS_TRI_OUT_POINTS : 0) | (rms ? PCS_TRI_OUT_RMS : 0) | (info ? PCS_TRI_OUT_INFO : 0) | (resid ? PCS_TRI_OUT_RESIDUALS : 0);
    if (want & ~t->refine_owned)
        return fail(PCS_ERR_STATE, "pcs_tri_refined: the last refinement wrote some of these outputs to caller buffers (or computed no residuals)");
    if (t->n_pts == 0) return PCS_OK;
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(tri_wait_done_host(t));   // the refinement may have been queued on a caller stream
    if (pts) HIPCHK(hipMemcpyAsync(pts, t->d_rpts, sizeof(double) * 3 * t->n_pts, hipMemcpyDeviceToHost, t->stream));
    if (rms) HIPCHK(hipMemcpyAsync(rms, t->d_rrms, sizeof(double) * 2 * t->n_pts, hipMemcpyDeviceToHost, t->stream));
    if (info) HIPCHK(hipMemcpyAsync(info, t->d_rinfo, sizeof(int32_t) * 3 * t->n_pts, hipMemcpyDeviceToHost, t->stream));
    if (resid && t->n_obs) HIPCHK(hipMemcpyAsync(resid, t->d_rres, sizeof(double) * 2 * t->n_obs, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return PCS_OK;
}

int pcs_tri_last_refine_ms(pcs_triangulator *t, float *kernel_ms) {
    if (!t || !kernel_ms) return fail(PCS_ERR_ARG, "pcs_tri_last_refine_ms: bad arguments");
    if (!t->refine_timed) return fail(PCS_ERR_STATE, "pcs_tri_last_refine_ms: no refinement has run yet");
    HIPCHK(hipEventSynchronize(t->r1));
    HIPCHK(hipEventElapsedTime(kernel_ms, t->r0, t->r1));
    return PCS_OK;
}

int pcs_tri_points(pcs_triangulator *t, double *pts) {
    if (!t || !pts) return fail(PCS_ERR_ARG, "pcs_tri_points: bad arguments");
    if (t->n_pts < 0 || (t->n_pts > 0 && (!t->out_owned || !t->d_pts || t->out_capacity < t->n_pts)))
        return fail(PCS_ERR_STATE, "pcs_tri_points: the last run left no handle-owned result (run with d_pts = NULL first)");
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(tri_wait_done_host(t));   // the run may have been queued on a caller stream
    if (t->n_pts) HIPCHK(hipMemcpyAsync(pts, t->d_pts, sizeof(double) * 3 * t->n_pts, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return PCS_OK;
}

int pcs_tri_synchronize(pcs_triangulator *t, void *stream) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_synchronize: bad arguments");
    HIPCHK(hipSetDevice(t->device));
    HIPCHK(hipStreamSynchronize(stream ? (hipStream_t)stream : t->stream));
    return PCS_OK;
}

int pcs_tri_last_kernel_ms(pcs_triangulator *t, float *kernel_ms) {
    if (!t || !kernel_ms) return fail(PCS_ERR_ARG, "pcs_tri_last_kernel_ms: bad arguments");
    if (!t->timed) return fail(PCS_ERR_STATE, "pcs_tri_last_kernel_ms: nothing has run yet");
    HIPCHK(hipEventSynchronize(t->e1));
    HIPCHK(hipEventElapsedTime(kernel_ms, t->e0, t->e1));
    return PCS_OK;
}

// stateless convenience form: one temporary handle per call (allocations + copies every time — use the handle API
// for repeated calls)
int pcs_triangulate(int device, int64_t n_obs, const int32_t *cam, const double *uv, int64_t n_pts, const int64_t *start_inds,
                    int64_t n_cams, const double *proj, const double *intrinsics, const double *dists, double *pts,
                    float *kernel_ms) {
    if (n_obs < 0 || n_pts < 0 || n_cams <= 0 || !start_inds || !proj || !intrinsics || !dists || (n_pts > 0 && !pts) ||
        (n_obs > 0 && (!cam || !uv)))
        return fail(PCS_ERR_ARG, "pcs_triangulate: bad arguments");
    if (n_pts == 0) return PCS_OK;
    pcs_triangulator *t = nullptr;
    int rc = pcs_tri_create(&t, device, n_cams);
    if (rc) return rc;
    rc = pcs_tri_set_cameras(t, proj, intrinsics, dists);
    if (!rc) rc = pcs_tri_set_observations(t, n_obs, cam, uv, n_pts, start_inds);
    if (!rc) rc = pcs_tri_run(t, nullptr, nullptr);
    if (!rc) rc = pcs_tri_points(t, pts);
    if (!rc && kernel_ms) rc = pcs_tri_last_kernel_ms(t, kernel_ms);
    const std::string keep = g_err;   // pcs_tri_destroy must not clobber the message
    pcs_tri_destroy(t);
    g_err = keep;
    return rc;
}
}  // extern "C"
