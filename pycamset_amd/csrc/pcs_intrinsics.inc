// pcs_intrinsics.inc — host side of the intrinsics estimation from planar views (included by pcs_engine.hip; kernels: ba_intrinsics.hpp).
// Fence, buffers and output slots are those of pcs_handle.inc (DESIGN.md, "Batched handles").
extern "C" {
// ---- intrinsics from planar views (SURVEY f6): a handle that owns the template, the observation copies and the outputs.
struct pcs_intrinsics_estimator {
    HandleCore core;
    KernelTimer timer;
    int64_t n_cams = 0, n_keys = 0;
    bool have_template = false;
    DevBuf pts;                            // template points
    DevBuf key, uv, start, cam_start;      // handle-owned copies of the observations; cam_start: the groups of camera c are [cam_start[c], cam_start[c + 1])
    DevBuf res;                            // (n_cams, 2) = (h, w), uploaded when a run brings other values than the last one
    std::vector<double> res_host;
    int64_t n_obs = 0, n_groups = -1;
    DevBuf intr, cinfo, eig, H, frame, ginfo, pix;   // handle-owned outputs
    int owned = 0;            // PCS_INTR_OUT_* bits: which outputs of the last run are handle-owned
    bool run_valid = false;   // a run since the template / observations were last set
};

int pcs_intr_create(pcs_intrinsics_estimator **out, int device, int64_t n_cams, int64_t n_keys) {
    if (!out || n_cams <= 0 || n_keys <= 0 || n_cams > INT32_MAX || n_keys > INT32_MAX) return fail(PCS_ERR_ARG, "pcs_intr_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_intr_create", device)) return rc;
    pcs_intrinsics_estimator *p = new pcs_intrinsics_estimator();
    p->n_cams = n_cams;
    p->n_keys = n_keys;
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->timer.create();
    if (e == hipSuccess) e = p->pts.alloc(n_keys * 3, sizeof(double));
    if (e == hipSuccess) e = p->res.alloc(n_cams * 2, sizeof(double));
    if (e == hipSuccess) e = p->cam_start.alloc(n_cams + 1, sizeof(int64_t));
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_intr_create: %s", hipGetErrorString(e));
        pcs_intr_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_intr_destroy(pcs_intrinsics_estimator *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->pts, &p->key, &p->uv, &p->start, &p->cam_start, &p->res, &p->intr, &p->cinfo, &p->eig, &p->H, &p->frame, &p->ginfo, &p->pix},
                    {&p->timer});
    delete p;
    return PCS_OK;
}

int pcs_intr_set_template(pcs_intrinsics_estimator *p, const double *points) {
    if (!p || !points) return fail(PCS_ERR_ARG, "pcs_intr_set_template: bad arguments");
    if (const int rc = set_fixed_array(p->core, p->pts, points, sizeof(double) * 3 * p->n_keys)) return rc;
    p->have_template = true;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_intr_set_observations(pcs_intrinsics_estimator *p, int64_t n_obs, const int32_t *key, const double *uv, int64_t n_groups, const int64_t *start_inds,
                              const int32_t *group_cam) {
    if (!p || n_obs < 0 || n_groups < 0 || n_groups > INT32_MAX || !start_inds || (n_obs > 0 && (!key || !uv)) || (n_groups > 0 && !group_cam))
        return fail(PCS_ERR_ARG, "pcs_intr_set_observations: bad arguments");
    std::vector<int64_t> cam_start((size_t)p->n_cams + 1, 0);
    const int bad = check_grouped_observations("pcs_intr_set_observations", n_obs, key, p->n_keys, n_groups, start_inds, [&](int64_t j) {
        if (const int rc = check_group_entity("group", j, "camera", group_cam[j], p->n_cams)) return rc;
        if (j > 0 && group_cam[j] < group_cam[j - 1]) return fail(PCS_ERR_ARG, "pcs_intr_set_observations: the groups must be sorted by camera");
        ++cam_start[group_cam[j] + 1];
        return (int)PCS_OK;
    });
    if (bad) return bad;
    for (int64_t c = 0; c < p->n_cams; ++c) cam_start[c + 1] += cam_start[c];
    HIPCHK(p->core.quiesce());
    p->n_groups = -1;
    const HostArray arrays[] = {{p->key, key, n_obs, sizeof(int32_t)}, {p->uv, uv, n_obs, 2 * sizeof(double)},
                                {p->start, start_inds, n_groups + 1, sizeof(int64_t)}, {p->cam_start, cam_start.data(), p->n_cams + 1, sizeof(int64_t)}};
    if (const int rc = upload_host_arrays(p->core, arrays, 4)) return rc;
    p->n_obs = n_obs;
    p->n_groups = n_groups;
    p->run_valid = false;
    return PCS_OK;
}

static_assert(INTR_NOT_ESTIMATED == PCS_INTR_NOT_ESTIMATED && INTR_FULL == PCS_INTR_FULL && INTR_FOCAL == PCS_INTR_FOCAL &&
              INTR_FOCAL_FALLBACK == PCS_INTR_FOCAL_FALLBACK && INTR_MODEL_FULL == PCS_INTR_MODEL_FULL && INTR_MODEL_FOCAL == PCS_INTR_MODEL_FOCAL &&
              INTR_GROUP_TOO_FEW == PCS_INTR_GROUP_TOO_FEW && INTR_GROUP_USED == PCS_INTR_GROUP_USED && INTR_GROUP_NOT_PLANAR == PCS_INTR_GROUP_NOT_PLANAR &&
              INTR_GROUP_NOT_FINITE == PCS_INTR_GROUP_NOT_FINITE && INTR_GROUP_FIT_FAILED == PCS_INTR_GROUP_FIT_FAILED, "status codes of pcs_hip.h");
// lanes per group and per camera (profiles/r12: kernel resources)
constexpr int INTR_G = 16;

// the outputs in the order of the PCS_INTR_OUT_* bits
enum { INTR_SLOT_INTR, INTR_SLOT_CINFO, INTR_SLOT_EIG, INTR_SLOT_H, INTR_SLOT_FRAME, INTR_SLOT_GINFO, INTR_SLOT_PIX, INTR_SLOTS };
static std::array<OutSlot, INTR_SLOTS> intr_out_slots(pcs_intrinsics_estimator *p, void *o_intr, void *o_cinfo, void *o_eig, void *o_H, void *o_frame,
                                                      void *o_ginfo, void *o_pix) {
    const int64_t nc = p->n_cams, ng = p->n_groups;
    return {{{PCS_INTR_OUT_INTR, p->intr, o_intr, nc, 9 * sizeof(double)}, {PCS_INTR_OUT_CAM_INFO, p->cinfo, o_cinfo, nc, 2 * sizeof(int32_t)},
             {PCS_INTR_OUT_EIG_RATIO, p->eig, o_eig, nc, sizeof(double)}, {PCS_INTR_OUT_HOMOGRAPHIES, p->H, o_H, ng, 9 * sizeof(double)},
             {PCS_INTR_OUT_FRAMES, p->frame, o_frame, ng, 9 * sizeof(double)}, {PCS_INTR_OUT_GROUP_INFO, p->ginfo, o_ginfo, ng, 2 * sizeof(int32_t)},
             {PCS_INTR_OUT_PIXEL_STATS, p->pix, o_pix, ng, 3 * sizeof(double)}}};
}

int pcs_intr_run(pcs_intrinsics_estimator *p, int model, int min_points, const double *res, double *d_intr, int32_t *d_cam_info, double *d_eig_ratio,
                 double *d_homographies, double *d_frames, int32_t *d_group_info, double *d_pixel_stats, void *stream) {
    if (model < PCS_INTR_MODEL_AUTO || model > PCS_INTR_MODEL_FOCAL || min_points < 4)
        return fail(PCS_ERR_ARG, "pcs_intr_run: bad options (model PCS_INTR_MODEL_*, min_points >= 4)");
    if (!p) return fail(PCS_ERR_ARG, "pcs_intr_run: NULL handle");
    if (!p->have_template || p->n_groups < 0) return fail(PCS_ERR_STATE, "pcs_intr_run: template or observations not set");
    if (res)
        for (int64_t k = 0; k < 2 * p->n_cams; ++k)
            if (!(res[k] > 0.0 && res[k] < INFINITY)) return fail(PCS_ERR_ARG, "pcs_intr_run: res must hold a finite (h, w) > 0 per camera");
    if (model == PCS_INTR_MODEL_AUTO) model = res ? PCS_INTR_MODEL_FOCAL : PCS_INTR_MODEL_FULL;   // OpenCV fixes the principal point when it knows the image size
    auto out = intr_out_slots(p, d_intr, d_cam_info, d_eig_ratio, d_homographies, d_frames, d_group_info, d_pixel_stats);
    const int64_t ng = p->n_groups, nc = p->n_cams;
    bool grows = false;
    const int owned = owned_slots(out.data(), INTR_SLOTS, &grows);
    HIPCHK(hipSetDevice(p->core.device));
    if (res && (p->res_host.size() != (size_t)(2 * nc) || std::memcmp(p->res_host.data(), res, sizeof(double) * 2 * nc) != 0)) {
        HIPCHK(p->core.quiesce());   // an earlier run may still read the old sizes
        HIPCHK(hipMemcpy(p->res.p, res, sizeof(double) * 2 * nc, hipMemcpyHostToDevice));
        p->res_host.assign(res, res + 2 * nc);
    }
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));   // outputs are shared between runs
    if (const int rc = grow_owned_slots(out.data(), INTR_SLOTS)) return rc;
    HIPCHK(hipEventRecord(p->timer.e0, s));   // after every allocation: nothing is queued by a call that fails in one
    double *d_H = out[INTR_SLOT_H].as<double>(), *d_pix = out[INTR_SLOT_PIX].as<double>();
    int32_t *d_ginfo = out[INTR_SLOT_GINFO].as<int32_t>();
    if (ng > 0)
        hipLaunchKernelGGL((intr_homography_kernel<INTR_G>), dim3((unsigned)((ng * INTR_G + 255) / 256)), dim3(256), 0, s, p->key.as<const int32_t>(),
                           p->uv.as<const double2>(), p->start.as<const int64_t>(), p->pts.as<const double>(), ng, min_points, d_H,
                           out[INTR_SLOT_FRAME].as<double>(), d_ginfo, d_pix);
    // a camera without groups still gets its NaN row and its status
    hipLaunchKernelGGL((intr_camera_kernel<INTR_G>), dim3((unsigned)((nc * INTR_G + 255) / 256)), dim3(256), 0, s, (const double *)d_H, (const int32_t *)d_ginfo,
                       (const double *)d_pix, p->cam_start.as<const int64_t>(), res ? p->res.as<const double>() : nullptr, nc, model,
                       out[INTR_SLOT_INTR].as<double>(), out[INTR_SLOT_CINFO].as<int32_t>(), out[INTR_SLOT_EIG].as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->timer.e1, s));
    p->timer.timed = true;
    p->owned = owned;
    p->run_valid = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_intr_results(pcs_intrinsics_estimator *p, double *intr, int32_t *cam_info, double *eig_ratio, double *homographies, double *frames,
                     int32_t *group_info, double *pixel_stats) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_intr_results: NULL handle");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_intr_results: no run on the current template and observations (pcs_intr_run first)");
    const auto out = intr_out_slots(p, intr, cam_info, eig_ratio, homographies, frames, group_info, pixel_stats);
    return fetch_slots(p->core, out.data(), INTR_SLOTS, p->owned, true, "pcs_intr_results", "the last run wrote some of these outputs to caller buffers");
}

int pcs_intr_last_kernel_ms(pcs_intrinsics_estimator *p, float *kernel_ms) {
    return timer_ms("pcs_intr_last_kernel_ms", p ? &p->timer : nullptr, kernel_ms, "nothing has run yet");
}
}  // extern "C"
