// pcs_pnp.inc — host side of the batched target-pose estimation (included by pcs_engine.hip; kernels: ba_pnp.hpp, ba_pnp_consensus.hpp).  Fence, buffers and
// output slots are those of pcs_handle.inc (DESIGN.md, "Batched handles").
extern "C" {
// ---- batched PnP (SURVEY f5): a handle that owns the camera table, the template, the observation copies and the outputs.
struct pcs_pose_estimator {
    HandleCore core;
    KernelTimer timer;
    int64_t n_cams = 0, n_keys = 0;
    bool have_cams = false, have_template = false;
    DevBuf tab, pts;                  // camera table (TRI_CAM_STRIDE doubles per camera), template points
    DevBuf key, vcam, uv, start;      // handle-owned copies of the observations (grown on demand)
    int64_t n_obs = 0, n_views = -1;
    DevBuf order, hist;               // views by observation count (enqueue_group_order), built by the first run of a set of observations
    bool order_valid = false;
    DevBuf pose, init, alt, rms, res, info;   // handle-owned outputs
    int owned = 0;            // PCS_PNP_OUT_* bits: which outputs of the last run are handle-owned
    bool run_valid = false;   // a run since the cameras / template / observations were last set
    // the consensus stage (pcs_pnp_set_consensus; kernels: ba_pnp_consensus.hpp).  n_hyp = 0: off, and none of these buffers exists.
    int cons_hyp = 0, cons_sample = 6;
    double cons_px = 8.0;
    uint64_t cons_seed = 0;
    bool cons_ran = false;                                  // the last run had the stage
    DevBuf s_key, s_uv, s_start, s_vcam, h_init, h_alt;     // the pseudo-views of the samples and their hypotheses
    DevBuf score, flag, cinfo, best;                        // (n_views, H, 2) scores; per observation flag; per view record and winning score
    DevBuf c_key, c_uv, c_start, c_order;                   // the table compacted to inliers and its visiting order
};

int pcs_pnp_create(pcs_pose_estimator **out, int device, int64_t n_cams, int64_t n_keys) {
    if (!out || n_cams <= 0 || n_keys <= 0 || n_cams > INT32_MAX || n_keys > INT32_MAX) return fail(PCS_ERR_ARG, "pcs_pnp_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_pnp_create", device)) return rc;
    pcs_pose_estimator *p = new pcs_pose_estimator();
    p->n_cams = n_cams;
    p->n_keys = n_keys;
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->timer.create();
    if (e == hipSuccess) e = p->tab.alloc(n_cams * TRI_CAM_STRIDE, sizeof(double));
    if (e == hipSuccess) e = p->pts.alloc(n_keys * 3, sizeof(double));
    if (e == hipSuccess) e = p->hist.alloc(GROUP_ORDER_HIST, sizeof(int32_t));
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
    p->core.destroy({&p->tab, &p->pts, &p->key, &p->vcam, &p->uv, &p->start, &p->order, &p->hist, &p->pose, &p->init, &p->alt, &p->rms, &p->res, &p->info,
                     &p->s_key, &p->s_uv, &p->s_start, &p->s_vcam, &p->h_init, &p->h_alt, &p->score, &p->flag, &p->cinfo, &p->best, &p->c_key, &p->c_uv,
                     &p->c_start, &p->c_order},
                    {&p->timer});
    delete p;
    return PCS_OK;
}

int pcs_pnp_set_cameras(pcs_pose_estimator *p, const double *intr) {
    if (!p || !intr) return fail(PCS_ERR_ARG, "pcs_pnp_set_cameras: bad arguments");
    std::vector<double> tab((size_t)p->n_cams * TRI_CAM_STRIDE, 0.0);
    for (int64_t c = 0; c < p->n_cams; ++c)
        for (int k = 0; k < 9; ++k) tab[c * TRI_CAM_STRIDE + 22 + k] = intr[9 * c + k];   // [fx cx fy cy k0 k1 p0 p1 k2]: the slab row as it is
    if (const int rc = set_fixed_array(p->core, p->tab, tab.data(), sizeof(double) * tab.size())) return rc;
    p->have_cams = true;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_pnp_set_template(pcs_pose_estimator *p, const double *points) {
    if (!p || !points) return fail(PCS_ERR_ARG, "pcs_pnp_set_template: bad arguments");
    if (const int rc = set_fixed_array(p->core, p->pts, points, sizeof(double) * 3 * p->n_keys)) return rc;
    p->have_template = true;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_pnp_set_observations(pcs_pose_estimator *p, int64_t n_obs, const int32_t *key, const double *uv, int64_t n_views, const int64_t *start_inds,
                             const int32_t *view_cam) {
    if (!p || n_obs < 0 || n_views < 0 || n_views > INT32_MAX || !start_inds || (n_obs > 0 && (!key || !uv)) || (n_views > 0 && !view_cam))
        return fail(PCS_ERR_ARG, "pcs_pnp_set_observations: bad arguments");
    if (const int rc = check_grouped_observations("pcs_pnp_set_observations", n_obs, key, p->n_keys, n_views, start_inds,
                                                  [&](int64_t j) { return check_group_entity("view", j, "camera", view_cam[j], p->n_cams); }))
        return rc;
    HIPCHK(p->core.quiesce());
    p->n_views = -1;
    const HostArray arrays[] = {{p->key, key, n_obs, sizeof(int32_t)}, {p->uv, uv, n_obs, 2 * sizeof(double)},
                                {p->start, start_inds, n_views + 1, sizeof(int64_t)}, {p->vcam, view_cam, n_views, sizeof(int32_t)}};
    if (const int rc = upload_host_arrays(p->core, arrays, 4)) return rc;
    p->n_obs = n_obs;
    p->n_views = n_views;
    p->order_valid = false;
    p->run_valid = false;
    return PCS_OK;
}

static_assert(PNP_NOT_ESTIMATED == PCS_PNP_NOT_ESTIMATED && PNP_CONVERGED == PCS_PNP_CONVERGED && PNP_MAX_ITER == PCS_PNP_MAX_ITER &&
              PNP_NO_DECREASE == PCS_PNP_NO_DECREASE, "status codes of pcs_hip.h");
// lanes per view, observations held in registers per lane (profiles/r10: kernel resources; profiles/r11: first times)
constexpr int PNP_G = 16, PNP_V = 4;
constexpr int PNP_CONS_MAX_HYP = 4096;   // hypotheses per view that pcs_pnp_set_consensus takes

// the outputs in the order of the PCS_PNP_OUT_* bits; the residuals last, so that a run without them takes the first five
enum { PNP_SLOT_POSE, PNP_SLOT_INIT, PNP_SLOT_ALT, PNP_SLOT_RMS, PNP_SLOT_INFO, PNP_SLOT_RESID, PNP_SLOTS };
static std::array<OutSlot, PNP_SLOTS> pnp_out_slots(pcs_pose_estimator *p, void *o_pose, void *o_init, void *o_alt, void *o_rms, void *o_info, void *o_resid) {
    const int64_t nv = p->n_views;
    return {{{PCS_PNP_OUT_POSE, p->pose, o_pose, nv, 6 * sizeof(double)}, {PCS_PNP_OUT_POSE_INIT, p->init, o_init, nv, 6 * sizeof(double)},
             {PCS_PNP_OUT_POSE_ALT, p->alt, o_alt, nv, 6 * sizeof(double)}, {PCS_PNP_OUT_RMS, p->rms, o_rms, nv, 2 * sizeof(double)},
             {PCS_PNP_OUT_INFO, p->info, o_info, nv, 3 * sizeof(int32_t)}, {PCS_PNP_OUT_RESIDUALS, p->res, o_resid, p->n_obs, 2 * sizeof(double)}}};
}

// The stage in front of the start and the LM (cv2.solvePnPRansac at the place of abstract_target.py:345-405).  Everything is checked
// before anything changes: a refused call keeps the previous setting.
int pcs_pnp_set_consensus(pcs_pose_estimator *p, int n_hypotheses, int sample_size, double inlier_px, uint64_t seed) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_pnp_set_consensus: NULL handle");
    if (n_hypotheses < 0 || n_hypotheses > PNP_CONS_MAX_HYP || sample_size < 4 || sample_size > CONS_MAX_SAMPLE || !std::isfinite(inlier_px) ||
        !(inlier_px > 0.0))
        return fail(PCS_ERR_ARG, "pcs_pnp_set_consensus: bad arguments (0 <= n_hypotheses <= %d, 4 <= sample_size <= %d, inlier_px finite and > 0)",
                    PNP_CONS_MAX_HYP, CONS_MAX_SAMPLE);
    p->cons_hyp = n_hypotheses;
    p->cons_sample = sample_size;
    p->cons_px = inlier_px;
    p->cons_seed = seed;
    return PCS_OK;
}

// The setting in force (cv2.solvePnPRansac's iterationsCount, sample, reprojectionError and seed, which OpenCV takes per call and does not keep).
int pcs_pnp_get_consensus(pcs_pose_estimator *p, int *n_hypotheses, int *sample_size, double *inlier_px, uint64_t *seed) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_pnp_get_consensus: NULL handle");
    if (n_hypotheses) *n_hypotheses = p->cons_hyp;
    if (sample_size) *sample_size = p->cons_sample;
    if (inlier_px) *inlier_px = p->cons_px;
    if (seed) *seed = p->cons_seed;
    return PCS_OK;
}

// A run with the consensus stage (cv2.solvePnPRansac for cv2.solvePnPGeneric, abstract_target.py:345-405): sample, hypotheses by the
// unchanged pnp_start_kernel on the pseudo-views, score, select, compact; then order, start and LM, unchanged, on the compacted table.
static int pnp_run_consensus(pcs_pose_estimator *p, int max_iter, double ftol, double xtol, double gtol, int min_points, bool want_resid,
                             std::array<OutSlot, PNP_SLOTS> &out, void *stream) {
    const int n_out = want_resid ? PNP_SLOTS : PNP_SLOTS - 1;
    const int64_t nv = p->n_views, H = p->cons_hyp, S = p->cons_sample, nh = nv * H, no = std::max<int64_t>(1, p->n_obs);
    if (nh > INT32_MAX / PNP_G) return fail(PCS_ERR_ARG, "pcs_pnp_run: %lld views x %lld hypotheses are more than one launch takes", (long long)nv, (long long)H);
    struct Need { DevBuf &buf; int64_t count; size_t bytes; };
    const Need need[] = {{p->s_key, nh * S, sizeof(int32_t)}, {p->s_uv, nh * S, 2 * sizeof(double)}, {p->s_start, nh + 1, sizeof(int64_t)},
                         {p->s_vcam, nh, sizeof(int32_t)}, {p->h_init, nh, 6 * sizeof(double)}, {p->h_alt, nh, 6 * sizeof(double)},
                         {p->score, nh, 2 * sizeof(double)}, {p->flag, no, sizeof(uint8_t)}, {p->cinfo, nv, 4 * sizeof(int32_t)},
                         {p->best, nv, sizeof(double)}, {p->c_key, no, sizeof(int32_t)}, {p->c_uv, no, 2 * sizeof(double)},
                         {p->c_start, nv + 1, sizeof(int64_t)}, {p->c_order, nv, sizeof(int32_t)}};
    bool grows = false;
    for (const Need &n : need) grows = grows || n.buf.grows(std::max<int64_t>(1, n.count));
    const int owned = owned_slots(out.data(), n_out, &grows);
    if (nv == 0) {
        p->owned = owned;
        p->run_valid = true;
        p->cons_ran = true;
        p->timer.timed = false;
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));
    int rc = grow_owned_slots(out.data(), n_out);
    for (const Need &n : need)
        if (!rc) rc = n.buf.grow(std::max<int64_t>(1, n.count), n.bytes);
    if (rc) return rc;
    HIPCHK(hipEventRecord(p->timer.e0, s));   // after every allocation: nothing is queued by a call that fails in one
    const int32_t *key = p->key.as<const int32_t>(), *vcam = p->vcam.as<const int32_t>();
    const double2 *uv = p->uv.as<const double2>();
    const int64_t *start = p->start.as<const int64_t>();
    const double *tab = p->tab.as<const double>(), *pts = p->pts.as<const double>();
    const double tau2 = p->cons_px * p->cons_px;
    const dim3 per_view((unsigned)((nv + 255) / 256)), view_groups((unsigned)((nv * PNP_G + 255) / 256)), hyp_groups((unsigned)((nh * PNP_G + 255) / 256));
    hipLaunchKernelGGL(pnp_sample_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, key, uv, start, vcam, nv, (int)H, (int)S, p->cons_seed,
                       p->s_key.as<int32_t>(), p->s_uv.as<double2>(), p->s_start.as<int64_t>(), p->s_vcam.as<int32_t>());
    hipLaunchKernelGGL((pnp_start_kernel<PNP_G>), hyp_groups, dim3(256), 0, s, p->s_key.as<const int32_t>(), p->s_uv.as<const double2>(),
                       p->s_start.as<const int64_t>(), p->s_vcam.as<const int32_t>(), tab, pts, nh, (const int32_t *)nullptr, (int)S, p->h_init.as<double>(),
                       p->h_alt.as<double>());
    hipLaunchKernelGGL((pnp_score_kernel<PNP_G, false>), hyp_groups, dim3(256), 0, s, key, uv, start, vcam, tab, pts, nv, (int)H, p->h_init.as<const double>(),
                       p->h_alt.as<const double>(), tau2, p->score.as<double>(), (double *)nullptr);
    hipLaunchKernelGGL((pnp_select_kernel<PNP_G>), view_groups, dim3(256), 0, s, key, uv, start, vcam, tab, pts, nv, (int)H, (int)S, p->h_init.as<const double>(),
                       p->h_alt.as<const double>(), p->score.as<const double>(), tau2, p->flag.as<uint8_t>(), p->cinfo.as<int32_t>(), p->best.as<double>());
    enqueue_compact_flagged<PNP_G>(key, uv, start, p->flag.as<const uint8_t>(), p->cinfo.as<const int32_t>(), nv, p->c_start.as<int64_t>(), p->c_key.as<int32_t>(),
                                   p->c_uv.as<double2>(), s);
    HIPCHK(hipGetLastError());
    if ((rc = enqueue_group_order(p->c_start.as<int64_t>(), nv, p->hist.as<int32_t>(), p->c_order.as<int32_t>(), s))) return rc;
    double *pose_init = out[PNP_SLOT_INIT].as<double>(), *pose_alt = out[PNP_SLOT_ALT].as<double>();
    hipLaunchKernelGGL((pnp_start_kernel<PNP_G>), view_groups, dim3(256), 0, s, p->c_key.as<const int32_t>(), p->c_uv.as<const double2>(),
                       p->c_start.as<const int64_t>(), vcam, tab, pts, nv, p->c_order.as<const int32_t>(), min_points, pose_init, pose_alt);
    hipLaunchKernelGGL((pnp_lm_kernel<PNP_G, PNP_V>), view_groups, dim3(256), 0, s, p->c_key.as<const int32_t>(), p->c_uv.as<const double2>(),
                       p->c_start.as<const int64_t>(), vcam, tab, pts, nv, p->c_order.as<const int32_t>(), (const double *)pose_init, (const double *)pose_alt,
                       max_iter, ftol, xtol, gtol, min_points, out[PNP_SLOT_POSE].as<double>(), out[PNP_SLOT_RMS].as<double>(), out[PNP_SLOT_INFO].as<int32_t>(),
                       (double *)nullptr);
    hipLaunchKernelGGL(cons_restore_count_kernel, per_view, dim3(256), 0, s, start, nv, out[PNP_SLOT_INFO].as<int32_t>(), 3, 2);
    if (want_resid)   // of ALL observations at the returned pose, outliers included: the one-candidate mode of the scoring kernel
        hipLaunchKernelGGL((pnp_score_kernel<PNP_G, true>), view_groups, dim3(256), 0, s, key, uv, start, vcam, tab, pts, nv, 1,
                           (const double *)out[PNP_SLOT_POSE].as<double>(), (const double *)nullptr, tau2, (double *)nullptr, out[PNP_SLOT_RESID].as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->timer.e1, s));
    p->timer.timed = true;
    p->owned = owned;
    p->run_valid = true;
    p->cons_ran = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_pnp_run(pcs_pose_estimator *p, int max_iter, double ftol, double xtol, double gtol, int min_points, int flags, double *d_pose,
                double *d_pose_init, double *d_pose_alt, double *d_rms, int32_t *d_info, double *d_resid, void *stream) {
    const bool rest_ok = min_points >= 1 && !(flags & ~PCS_PNP_RESIDUALS);
    if (const int rc = check_lm_options("pcs_pnp_run", max_iter, ftol, xtol, gtol, rest_ok, "min_points >= 1, flags PCS_PNP_RESIDUALS")) return rc;
    if (!p) return fail(PCS_ERR_ARG, "pcs_pnp_run: NULL handle");
    if (!p->have_cams || !p->have_template || p->n_views < 0) return fail(PCS_ERR_STATE, "pcs_pnp_run: cameras, template or observations not set");
    const bool want_resid = flags & PCS_PNP_RESIDUALS;
    auto out = pnp_out_slots(p, d_pose, d_pose_init, d_pose_alt, d_rms, d_info, d_resid);
    if (p->cons_hyp > 0) return pnp_run_consensus(p, max_iter, ftol, xtol, gtol, min_points, want_resid, out, stream);
    p->cons_ran = false;
    const int n_out = want_resid ? PNP_SLOTS : PNP_SLOTS - 1;
    const int64_t nv = p->n_views;
    bool grows = !p->order_valid && p->order.grows(nv);
    const int owned = owned_slots(out.data(), n_out, &grows);
    if (nv == 0) {
        p->owned = owned;
        p->run_valid = true;
        p->timer.timed = false;   // nothing ran: no time of an earlier run is reported for this one
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));   // outputs and the order are shared between runs
    int rc = grow_owned_slots(out.data(), n_out);
    if (!rc && !p->order_valid) rc = p->order.grow(nv, sizeof(int32_t));
    if (rc) return rc;
    HIPCHK(hipEventRecord(p->timer.e0, s));   // after every allocation: nothing is queued by a call that fails in one
    if (!p->order_valid) {
        if ((rc = enqueue_group_order(p->start.as<int64_t>(), nv, p->hist.as<int32_t>(), p->order.as<int32_t>(), s))) return rc;
        p->order_valid = true;
    }
    double *pose_init = out[PNP_SLOT_INIT].as<double>(), *pose_alt = out[PNP_SLOT_ALT].as<double>();
    const dim3 grid((unsigned)((nv * PNP_G + 255) / 256));
    hipLaunchKernelGGL((pnp_start_kernel<PNP_G>), grid, dim3(256), 0, s, p->key.as<const int32_t>(), p->uv.as<const double2>(), p->start.as<const int64_t>(),
                       p->vcam.as<const int32_t>(), p->tab.as<const double>(), p->pts.as<const double>(), nv, p->order.as<const int32_t>(), min_points, pose_init, pose_alt);
    hipLaunchKernelGGL((pnp_lm_kernel<PNP_G, PNP_V>), grid, dim3(256), 0, s, p->key.as<const int32_t>(), p->uv.as<const double2>(), p->start.as<const int64_t>(),
                       p->vcam.as<const int32_t>(), p->tab.as<const double>(), p->pts.as<const double>(), nv, p->order.as<const int32_t>(), (const double *)pose_init,
                       (const double *)pose_alt, max_iter, ftol, xtol, gtol, min_points, out[PNP_SLOT_POSE].as<double>(), out[PNP_SLOT_RMS].as<double>(),
                       out[PNP_SLOT_INFO].as<int32_t>(), want_resid ? out[PNP_SLOT_RESID].as<double>() : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->timer.e1, s));
    p->timer.timed = true;
    p->owned = owned;
    p->run_valid = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_pnp_results(pcs_pose_estimator *p, double *pose, double *pose_init, double *pose_alt, double *rms, int32_t *info, double *resid) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_pnp_results: NULL handle");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_pnp_results: no run on the current cameras, template and observations (pcs_pnp_run first)");
    const auto out = pnp_out_slots(p, pose, pose_init, pose_alt, rms, info, resid);
    return fetch_slots(p->core, out.data(), PNP_SLOTS, p->owned, p->n_views != 0, "pcs_pnp_results",
                       "the last run wrote some of these outputs to caller buffers (or computed no residuals)");
}

// What the consensus stage of the last run found (cv2.solvePnPRansac's inlier list): blocking, any pointer may be NULL.
int pcs_pnp_consensus_results(pcs_pose_estimator *p, uint8_t *inlier, int32_t *cinfo, double *score) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_pnp_consensus_results: NULL handle");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_pnp_consensus_results: no run on the current cameras, template and observations (pcs_pnp_run first)");
    if (!p->cons_ran) return fail(PCS_ERR_STATE, "pcs_pnp_consensus_results: the last run had no consensus stage (pcs_pnp_set_consensus)");
    const OutSlot out[] = {{1, p->flag, inlier, p->n_obs, sizeof(uint8_t)}, {2, p->cinfo, cinfo, p->n_views, 4 * sizeof(int32_t)},
                           {4, p->best, score, p->n_views, sizeof(double)}};
    return fetch_slots(p->core, out, 3, 7, p->n_views != 0, "pcs_pnp_consensus_results", "");
}

int pcs_pnp_last_kernel_ms(pcs_pose_estimator *p, float *kernel_ms) {
    return timer_ms("pcs_pnp_last_kernel_ms", p ? &p->timer : nullptr, kernel_ms, "nothing has run yet");
}
}  // extern "C"
