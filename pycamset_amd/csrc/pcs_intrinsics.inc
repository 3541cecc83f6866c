// pcs_intrinsics.inc — host side of the intrinsics estimation from planar views (included by pcs_engine.hip; kernels: ba_intrinsics.hpp,
// ba_intr_consensus.hpp).
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
    // the consensus stage (pcs_intr_set_consensus; kernels: ba_intr_consensus.hpp).  cons_hyp = 0: off, and none of these buffers exists.
    int cons_hyp = 0, cons_sample = 6;
    double cons_px = 8.0;
    uint64_t cons_seed = 0;
    bool cons_ran = false;                                  // the last run had the stage
    std::vector<int32_t> gcam_host;                         // the camera of every group: it reaches the device with the first run that has the stage
    bool gcam_valid = false;
    DevBuf gcam;
    DevBuf s_key, s_uv, s_start, s_gcam;                    // the pseudo-groups of the samples
    DevBuf h_H, h_frame, h_info, h_pix;                     // their homographies, frames, statuses and pixel statistics
    DevBuf score, flag, consinfo, best;                     // (n_groups, H) scores; per observation flag; per group record and winning score
    DevBuf c_key, c_uv, c_start;                            // the table compacted to inliers
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
    p->core.destroy({&p->pts, &p->key, &p->uv, &p->start, &p->cam_start, &p->res, &p->intr, &p->cinfo, &p->eig, &p->H, &p->frame, &p->ginfo, &p->pix,
                     &p->gcam, &p->s_key, &p->s_uv, &p->s_start, &p->s_gcam, &p->h_H, &p->h_frame, &p->h_info, &p->h_pix, &p->score, &p->flag, &p->consinfo,
                     &p->best, &p->c_key, &p->c_uv, &p->c_start},
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
    p->gcam_host.assign(group_cam, group_cam + n_groups);
    p->gcam_valid = false;
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

constexpr int INTR_CONS_MAX_HYP = 4096;   // hypotheses per group that pcs_intr_set_consensus takes

// The stage in front of the homographies (cv2.findHomography's RANSAC at the place of abstract_target.py:263-343).  Everything is checked
// before anything changes: a refused call keeps the previous setting.
int pcs_intr_set_consensus(pcs_intrinsics_estimator *p, int n_hypotheses, int sample_size, double inlier_px, uint64_t seed) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_intr_set_consensus: NULL handle");
    if (n_hypotheses < 0 || n_hypotheses > INTR_CONS_MAX_HYP || sample_size < 4 || sample_size > CONS_MAX_SAMPLE || !std::isfinite(inlier_px) ||
        !(inlier_px > 0.0))
        return fail(PCS_ERR_ARG, "pcs_intr_set_consensus: bad arguments (0 <= n_hypotheses <= %d, 4 <= sample_size <= %d, inlier_px finite and > 0)",
                    INTR_CONS_MAX_HYP, CONS_MAX_SAMPLE);
    p->cons_hyp = n_hypotheses;
    p->cons_sample = sample_size;
    p->cons_px = inlier_px;
    p->cons_seed = seed;
    return PCS_OK;
}

// The setting in force (cv2.findHomography's maxIters, the sample, ransacReprojThreshold and a seed, which OpenCV takes per call and does not keep).
int pcs_intr_get_consensus(pcs_intrinsics_estimator *p, int *n_hypotheses, int *sample_size, double *inlier_px, uint64_t *seed) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_intr_get_consensus: NULL handle");
    if (n_hypotheses) *n_hypotheses = p->cons_hyp;
    if (sample_size) *sample_size = p->cons_sample;
    if (inlier_px) *inlier_px = p->cons_px;
    if (seed) *seed = p->cons_seed;
    return PCS_OK;
}

// A run with the consensus stage: sample, hypotheses by the unchanged intr_homography_kernel on the pseudo-groups, score, select, compact;
// then the homography and camera kernels, unchanged, on the compacted table, and the observation counts back into group_info.
static int intr_run_consensus(pcs_intrinsics_estimator *p, int model, int min_points, const double *d_res, std::array<OutSlot, INTR_SLOTS> &out, void *stream) {
    const int64_t ng = p->n_groups, nc = p->n_cams, H = p->cons_hyp, S = p->cons_sample, nh = ng * H, no = std::max<int64_t>(1, p->n_obs);
    if (nh > INT32_MAX / INTR_G) return fail(PCS_ERR_ARG, "pcs_intr_run: %lld groups x %lld hypotheses are more than one launch takes", (long long)ng, (long long)H);
    struct Need { DevBuf &buf; int64_t count; size_t bytes; };
    const Need need[] = {{p->gcam, ng, sizeof(int32_t)}, {p->s_key, nh * S, sizeof(int32_t)}, {p->s_uv, nh * S, 2 * sizeof(double)},
                         {p->s_start, nh + 1, sizeof(int64_t)}, {p->s_gcam, nh, sizeof(int32_t)}, {p->h_H, nh, 9 * sizeof(double)},
                         {p->h_frame, nh, 9 * sizeof(double)}, {p->h_info, nh, 2 * sizeof(int32_t)}, {p->h_pix, nh, 3 * sizeof(double)},
                         {p->score, nh, sizeof(double)}, {p->flag, no, sizeof(uint8_t)}, {p->consinfo, ng, 4 * sizeof(int32_t)},
                         {p->best, ng, sizeof(double)}, {p->c_key, no, sizeof(int32_t)}, {p->c_uv, no, 2 * sizeof(double)},
                         {p->c_start, ng + 1, sizeof(int64_t)}};
    bool grows = false;
    for (const Need &n : need) grows = grows || n.buf.grows(std::max<int64_t>(1, n.count));
    const int owned = owned_slots(out.data(), INTR_SLOTS, &grows);
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));   // outputs and the stage's buffers are shared between runs
    int rc = grow_owned_slots(out.data(), INTR_SLOTS);
    for (const Need &n : need)
        if (!rc) rc = n.buf.grow(std::max<int64_t>(1, n.count), n.bytes);
    if (rc) return rc;
    HIPCHK(hipEventRecord(p->timer.e0, s));   // after every allocation: nothing is queued by a call that fails in one
    double *d_H = out[INTR_SLOT_H].as<double>(), *d_pix = out[INTR_SLOT_PIX].as<double>();
    int32_t *d_ginfo = out[INTR_SLOT_GINFO].as<int32_t>();
    if (ng > 0) {
        if (!p->gcam_valid) {   // gcam_host lives until the next pcs_intr_set_observations, which waits for this run first
            HIPCHK(hipMemcpyAsync(p->gcam.p, p->gcam_host.data(), sizeof(int32_t) * (size_t)ng, hipMemcpyHostToDevice, s));
            p->gcam_valid = true;
        }
        const int32_t *key = p->key.as<const int32_t>();
        const double2 *uv = p->uv.as<const double2>();
        const int64_t *start = p->start.as<const int64_t>();
        const double *pts = p->pts.as<const double>();
        const double tau2 = p->cons_px * p->cons_px;
        const dim3 per_group((unsigned)((ng + 255) / 256)), groups((unsigned)((ng * INTR_G + 255) / 256)), hyp_groups((unsigned)((nh * INTR_G + 255) / 256));
        hipLaunchKernelGGL(pnp_sample_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, key, uv, start, p->gcam.as<const int32_t>(), ng, (int)H, (int)S,
                           p->cons_seed, p->s_key.as<int32_t>(), p->s_uv.as<double2>(), p->s_start.as<int64_t>(), p->s_gcam.as<int32_t>());
        hipLaunchKernelGGL((intr_homography_kernel<INTR_G>), hyp_groups, dim3(256), 0, s, p->s_key.as<const int32_t>(), p->s_uv.as<const double2>(),
                           p->s_start.as<const int64_t>(), pts, nh, (int)S, p->h_H.as<double>(), p->h_frame.as<double>(), p->h_info.as<int32_t>(),
                           p->h_pix.as<double>());
        hipLaunchKernelGGL((intr_score_kernel<INTR_G>), hyp_groups, dim3(256), 0, s, key, uv, start, pts, ng, (int)H, p->h_H.as<const double>(),
                           p->h_frame.as<const double>(), p->h_info.as<const int32_t>(), tau2, p->score.as<double>());
        hipLaunchKernelGGL((intr_select_kernel<INTR_G>), groups, dim3(256), 0, s, key, uv, start, pts, ng, (int)H, (int)std::max<int64_t>(S, min_points),
                           p->h_H.as<const double>(), p->h_frame.as<const double>(), p->score.as<const double>(), tau2, p->flag.as<uint8_t>(),
                           p->consinfo.as<int32_t>(), p->best.as<double>());
        enqueue_compact_flagged<INTR_G>(key, uv, start, p->flag.as<const uint8_t>(), p->consinfo.as<const int32_t>(), ng, p->c_start.as<int64_t>(),
                                        p->c_key.as<int32_t>(), p->c_uv.as<double2>(), s);
        hipLaunchKernelGGL((intr_homography_kernel<INTR_G>), groups, dim3(256), 0, s, p->c_key.as<const int32_t>(), p->c_uv.as<const double2>(),
                           p->c_start.as<const int64_t>(), pts, ng, min_points, d_H, out[INTR_SLOT_FRAME].as<double>(), d_ginfo, d_pix);
    }
    // the camera kernel sees the inlier counts: its pixel centroid weights by them, as the plain run on the inlier rows does
    hipLaunchKernelGGL((intr_camera_kernel<INTR_G>), dim3((unsigned)((nc * INTR_G + 255) / 256)), dim3(256), 0, s, (const double *)d_H, (const int32_t *)d_ginfo,
                       (const double *)d_pix, p->cam_start.as<const int64_t>(), d_res, nc, model, out[INTR_SLOT_INTR].as<double>(),
                       out[INTR_SLOT_CINFO].as<int32_t>(), out[INTR_SLOT_EIG].as<double>());
    if (ng > 0)
        hipLaunchKernelGGL(cons_restore_count_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, p->start.as<const int64_t>(), ng, d_ginfo, 2, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->timer.e1, s));
    p->timer.timed = true;
    p->owned = owned;
    p->run_valid = true;
    p->cons_ran = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
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
    if (p->cons_hyp > 0) return intr_run_consensus(p, model, min_points, res ? p->res.as<const double>() : nullptr, out, stream);
    p->cons_ran = false;
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

// What the consensus stage of the last run found (cv2.findHomography's mask): blocking, any pointer may be NULL.
int pcs_intr_consensus_results(pcs_intrinsics_estimator *p, uint8_t *inlier, int32_t *cinfo, double *score) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_intr_consensus_results: NULL handle");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_intr_consensus_results: no run on the current template and observations (pcs_intr_run first)");
    if (!p->cons_ran) return fail(PCS_ERR_STATE, "pcs_intr_consensus_results: the last run had no consensus stage (pcs_intr_set_consensus)");
    const OutSlot out[] = {{1, p->flag, inlier, p->n_obs, sizeof(uint8_t)}, {2, p->consinfo, cinfo, p->n_groups, 4 * sizeof(int32_t)},
                           {4, p->best, score, p->n_groups, sizeof(double)}};
    return fetch_slots(p->core, out, 3, 7, p->n_groups != 0, "pcs_intr_consensus_results", "");
}

int pcs_intr_last_kernel_ms(pcs_intrinsics_estimator *p, float *kernel_ms) {
    return timer_ms("pcs_intr_last_kernel_ms", p ? &p->timer : nullptr, kernel_ms, "nothing has run yet");
}
}  // extern "C"
