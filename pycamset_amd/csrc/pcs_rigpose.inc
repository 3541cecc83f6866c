// pcs_rigpose.inc — host side of the per-image target pose in a calibrated rig (included by pcs_engine.hip; kernel: ba_rigpose.hpp).
// Fence, buffers and output slots are those of pcs_handle.inc (DESIGN.md, "Batched handles").
extern "C" {
// ---- rig localiser (SURVEY f9): a handle that owns the camera and extrinsic tables, the template, the observation copies, the start
// poses and the outputs.
struct pcs_rig_localiser {
    HandleCore core;
    KernelTimer timer;
    int64_t n_cams = 0, n_keys = 0;
    bool have_cams = false, have_extr = false, have_template = false, have_start = false;
    DevBuf tab, ext, pts;             // camera table (TRI_CAM_STRIDE doubles per camera), extrinsics (12 per camera), template points
    DevBuf key, cam, uv, start;       // handle-owned copies of the observations (grown on demand)
    DevBuf pose0;                     // the start poses (n_groups, 6)
    int64_t n_obs = 0, n_groups = -1;
    DevBuf order, hist;               // images by observation count (enqueue_group_order), built by the first run of a set of observations
    bool order_valid = false;
    DevBuf pose, rms, info, hess, res;   // handle-owned outputs
    DevBuf cost;                         // (n_groups, 2) 0.5 sum rho0 at the pose and at the start of the last run: always handle-owned
    LinearCosts lin;                     // a linear run derives them in pcs_rigpose_costs
    HandleLoss loss;                     // pcs_rigpose_set_loss: the handle's, whatever cameras and observations follow
    int owned = 0;            // PCS_RIGPOSE_OUT_* bits: which outputs of the last run are handle-owned
    bool run_valid = false;   // a run since the inputs were last set
};

int pcs_rigpose_create(pcs_rig_localiser **out, int device, int64_t n_cams, int64_t n_keys) {
    if (!out || n_cams <= 0 || n_keys <= 0 || n_cams > INT32_MAX || n_keys > INT32_MAX) return fail(PCS_ERR_ARG, "pcs_rigpose_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_rigpose_create", device)) return rc;
    pcs_rig_localiser *p = new pcs_rig_localiser();
    p->n_cams = n_cams;
    p->n_keys = n_keys;
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->timer.create();
    if (e == hipSuccess) e = p->tab.alloc(n_cams * TRI_CAM_STRIDE, sizeof(double));
    if (e == hipSuccess) e = p->ext.alloc(n_cams * RIGPOSE_EXT_STRIDE, sizeof(double));
    if (e == hipSuccess) e = p->pts.alloc(n_keys * 3, sizeof(double));
    if (e == hipSuccess) e = p->hist.alloc(GROUP_ORDER_HIST, sizeof(int32_t));
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_rigpose_create: %s", hipGetErrorString(e));
        pcs_rigpose_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_rigpose_destroy(pcs_rig_localiser *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->tab, &p->ext, &p->pts, &p->key, &p->cam, &p->uv, &p->start, &p->pose0, &p->order, &p->hist, &p->pose, &p->rms, &p->info, &p->hess,
                     &p->res, &p->cost},
                    {&p->timer});
    delete p;
    return PCS_OK;
}

int pcs_rigpose_set_cameras(pcs_rig_localiser *p, const double *intr) {
    if (!p || !intr) return fail(PCS_ERR_ARG, "pcs_rigpose_set_cameras: bad arguments");
    std::vector<double> tab((size_t)p->n_cams * TRI_CAM_STRIDE, 0.0);
    for (int64_t c = 0; c < p->n_cams; ++c)
        for (int k = 0; k < 9; ++k) tab[c * TRI_CAM_STRIDE + 22 + k] = intr[9 * c + k];   // [fx cx fy cy k0 k1 p0 p1 k2]: the slab row as it is
    if (const int rc = set_fixed_array(p->core, p->tab, tab.data(), sizeof(double) * tab.size())) return rc;
    p->have_cams = true;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_rigpose_set_extrinsics(pcs_rig_localiser *p, const double *ext) {
    if (!p || !ext) return fail(PCS_ERR_ARG, "pcs_rigpose_set_extrinsics: bad arguments");
    if (const int rc = set_fixed_array(p->core, p->ext, ext, sizeof(double) * RIGPOSE_EXT_STRIDE * p->n_cams)) return rc;
    p->have_extr = true;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_rigpose_set_template(pcs_rig_localiser *p, const double *points) {
    if (!p || !points) return fail(PCS_ERR_ARG, "pcs_rigpose_set_template: bad arguments");
    if (const int rc = set_fixed_array(p->core, p->pts, points, sizeof(double) * 3 * p->n_keys)) return rc;
    p->have_template = true;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_rigpose_set_observations(pcs_rig_localiser *p, int64_t n_obs, const int32_t *key, const int32_t *cam, const double *uv, int64_t n_groups,
                                 const int64_t *start_inds) {
    if (n_obs < 0 || n_groups < 0 || n_groups > INT32_MAX || !start_inds || (n_obs > 0 && (!key || !cam || !uv)))
        return fail(PCS_ERR_ARG, "pcs_rigpose_set_observations: bad arguments");
    // the shape of the table needs no handle: start_inds, and the camera column sorted inside every group (the first bad group decides)
    if (start_inds[0] != 0 || start_inds[n_groups] != n_obs) return fail(PCS_ERR_ARG, "pcs_rigpose_set_observations: start_inds must run from 0 to n_obs");
    for (int64_t j = 0; j < n_groups; ++j) {
        if (start_inds[j + 1] < start_inds[j] || start_inds[j + 1] > n_obs)
            return fail(PCS_ERR_ARG, "pcs_rigpose_set_observations: start_inds must be non-decreasing");
        for (int64_t r = start_inds[j] + 1; r < start_inds[j + 1]; ++r)
            if (cam[r] < cam[r - 1])
                return fail(PCS_ERR_ARG, "pcs_rigpose_set_observations: cam must be non-decreasing inside a group (group %lld, observation %lld)", (long long)j,
                            (long long)r);
    }
    if (!p) return fail(PCS_ERR_ARG, "pcs_rigpose_set_observations: NULL handle");
    if (const int rc = check_grouped_observations("pcs_rigpose_set_observations", n_obs, key, p->n_keys, n_groups, start_inds, [&](int64_t j) {
            if (start_inds[j + 1] == start_inds[j]) return (int)PCS_OK;   // sorted: the ends of the run bound it
            if (const int rc = check_group_entity("group", j, "camera", cam[start_inds[j]], p->n_cams)) return rc;
            return check_group_entity("group", j, "camera", cam[start_inds[j + 1] - 1], p->n_cams);
        }))
        return rc;
    HIPCHK(p->core.quiesce());
    p->n_groups = -1;
    p->have_start = false;
    const HostArray arrays[] = {{p->key, key, n_obs, sizeof(int32_t)}, {p->cam, cam, n_obs, sizeof(int32_t)}, {p->uv, uv, n_obs, 2 * sizeof(double)},
                                {p->start, start_inds, n_groups + 1, sizeof(int64_t)}};
    if (const int rc = upload_host_arrays(p->core, arrays, 4)) return rc;
    p->n_obs = n_obs;
    p->n_groups = n_groups;
    p->order_valid = false;
    p->run_valid = false;
    return PCS_OK;
}

int pcs_rigpose_set_start(pcs_rig_localiser *p, const double *poses) {
    if (!p || !poses) return fail(PCS_ERR_ARG, "pcs_rigpose_set_start: bad arguments");
    if (p->n_groups < 0) return fail(PCS_ERR_STATE, "pcs_rigpose_set_start: observations not set (they give the number of poses)");
    HIPCHK(p->core.quiesce());
    const HostArray arrays[] = {{p->pose0, poses, 6 * p->n_groups, sizeof(double)}};
    if (const int rc = upload_host_arrays(p->core, arrays, 1)) return rc;
    p->have_start = true;
    p->run_valid = false;
    return PCS_OK;
}

static_assert(PNP_NOT_ESTIMATED == PCS_RIGPOSE_NOT_ESTIMATED && PNP_CONVERGED == PCS_RIGPOSE_CONVERGED && PNP_MAX_ITER == PCS_RIGPOSE_MAX_ITER &&
              PNP_NO_DECREASE == PCS_RIGPOSE_NO_DECREASE, "status codes of pcs_hip.h");
// Lanes per image when the caller leaves the width open: 64 from this mean number of observations per image on.  Measured at 2 000
// images (profiles/r17/README.md, "Width rule"): 16 lanes are faster at a mean of 96 and, by 5 %, at 192; 64 lanes at 384 and above.
constexpr int64_t RIGPOSE_WIDE_FROM = 256;

enum { RIGPOSE_SLOT_POSE, RIGPOSE_SLOT_RMS, RIGPOSE_SLOT_INFO, RIGPOSE_SLOT_HESS, RIGPOSE_SLOT_RESID, RIGPOSE_SLOTS };
static std::array<OutSlot, RIGPOSE_SLOTS> rigpose_out_slots(pcs_rig_localiser *p, void *o_pose, void *o_rms, void *o_info, void *o_hess, void *o_resid) {
    const int64_t ng = p->n_groups;
    return {{{PCS_RIGPOSE_OUT_POSE, p->pose, o_pose, ng, 6 * sizeof(double)}, {PCS_RIGPOSE_OUT_RMS, p->rms, o_rms, ng, 2 * sizeof(double)},
             {PCS_RIGPOSE_OUT_INFO, p->info, o_info, ng, 4 * sizeof(int32_t)}, {PCS_RIGPOSE_OUT_HESSIAN, p->hess, o_hess, ng, RIGPOSE_HESS * sizeof(double)},
             {PCS_RIGPOSE_OUT_RESIDUALS, p->res, o_resid, p->n_obs, 2 * sizeof(double)}}};
}

}  // extern "C"

// PCS_LOSS_LINEAR launches the kernel a handle without a loss always launched; any other kind its robust twin, which writes the costs itself
template <int G>
static void rigpose_launch(pcs_rig_localiser *p, hipStream_t s, int max_iter, double ftol, double xtol, double gtol, int min_points, const OutSlot *out,
                           bool want_resid) {
    const int64_t ng = p->n_groups;
    const dim3 grid((unsigned)((ng * G + 255) / 256));
    if (p->loss.kind == PCS_LOSS_LINEAR)
        hipLaunchKernelGGL((rigpose_lm_kernel<G>), grid, dim3(256), 0, s, p->key.as<const int32_t>(), p->cam.as<const int32_t>(),
                           p->uv.as<const double2>(), p->start.as<const int64_t>(), p->tab.as<const double>(), p->ext.as<const double>(),
                           p->pts.as<const double>(), ng, p->order.as<const int32_t>(), p->pose0.as<const double>(), max_iter, ftol, xtol, gtol, min_points,
                           out[RIGPOSE_SLOT_POSE].as<double>(), out[RIGPOSE_SLOT_RMS].as<double>(), out[RIGPOSE_SLOT_INFO].as<int32_t>(),
                           out[RIGPOSE_SLOT_HESS].as<double>(), want_resid ? out[RIGPOSE_SLOT_RESID].as<double>() : nullptr);
    else
        hipLaunchKernelGGL((rigpose_lm_kernel<G, GroupLoss, double *>), grid, dim3(256), 0, s, p->key.as<const int32_t>(), p->cam.as<const int32_t>(),
                           p->uv.as<const double2>(), p->start.as<const int64_t>(), p->tab.as<const double>(), p->ext.as<const double>(),
                           p->pts.as<const double>(), ng, p->order.as<const int32_t>(), p->pose0.as<const double>(), max_iter, ftol, xtol, gtol, min_points,
                           out[RIGPOSE_SLOT_POSE].as<double>(), out[RIGPOSE_SLOT_RMS].as<double>(), out[RIGPOSE_SLOT_INFO].as<int32_t>(),
                           out[RIGPOSE_SLOT_HESS].as<double>(), want_resid ? out[RIGPOSE_SLOT_RESID].as<double>() : nullptr, p->loss.args(),
                           p->cost.as<double>());
}

extern "C" {

int pcs_rigpose_run(pcs_rig_localiser *p, int max_iter, double ftol, double xtol, double gtol, int min_points, int group_lanes, int flags, double *d_pose,
                    double *d_rms, int32_t *d_info, double *d_hess, double *d_resid, void *stream) {
    const bool rest_ok = min_points >= 1 && (group_lanes == 0 || group_lanes == 16 || group_lanes == 64) && !(flags & ~PCS_RIGPOSE_RESIDUALS);
    if (const int rc = check_lm_options("pcs_rigpose_run", max_iter, ftol, xtol, gtol, rest_ok,
                                        "min_points >= 1, group_lanes 0, 16 or 64, flags PCS_RIGPOSE_RESIDUALS"))
        return rc;
    if (!p) return fail(PCS_ERR_ARG, "pcs_rigpose_run: NULL handle");
    if (!p->have_cams || !p->have_extr || !p->have_template || p->n_groups < 0 || !p->have_start)
        return fail(PCS_ERR_STATE, "pcs_rigpose_run: cameras, extrinsics, template, observations or start poses not set");
    const bool want_resid = flags & PCS_RIGPOSE_RESIDUALS;
    auto out = rigpose_out_slots(p, d_pose, d_rms, d_info, d_hess, d_resid);
    const int n_out = want_resid ? RIGPOSE_SLOTS : RIGPOSE_SLOTS - 1;
    const int64_t ng = p->n_groups;
    const bool robust = p->loss.kind != PCS_LOSS_LINEAR;
    bool grows = (!p->order_valid && p->order.grows(ng)) || (robust && p->cost.grows(ng));
    const int owned = owned_slots(out.data(), n_out, &grows);
    if (ng == 0) {
        p->owned = owned;
        p->lin.pending = false;
        p->run_valid = true;
        p->timer.timed = false;   // nothing ran: no time of an earlier run is reported for this one
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));   // outputs and the order are shared between runs
    int rc = grow_owned_slots(out.data(), n_out);
    if (!rc && !p->order_valid) rc = p->order.grow(ng, sizeof(int32_t));
    if (!rc && robust) rc = p->cost.grow(ng, 2 * sizeof(double));
    if (rc) return rc;
    HIPCHK(hipEventRecord(p->timer.e0, s));   // after every allocation: nothing is queued by a call that fails in one
    if (!p->order_valid) {
        if ((rc = enqueue_group_order(p->start.as<int64_t>(), ng, p->hist.as<int32_t>(), p->order.as<int32_t>(), s))) return rc;
        p->order_valid = true;
    }
    const int lanes = group_lanes ? group_lanes : (p->n_obs >= RIGPOSE_WIDE_FROM * ng ? 64 : 16);
    if (lanes == 64) rigpose_launch<64>(p, s, max_iter, ftol, xtol, gtol, min_points, out.data(), want_resid);
    else rigpose_launch<16>(p, s, max_iter, ftol, xtol, gtol, min_points, out.data(), want_resid);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->timer.e1, s));
    p->lin = {out[RIGPOSE_SLOT_RMS].as<double>(), p->start.as<int64_t>(), !robust};
    p->timer.timed = true;
    p->owned = owned;
    p->run_valid = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_rigpose_results(pcs_rig_localiser *p, double *pose, double *rms, int32_t *info, double *hess, double *resid) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_rigpose_results: NULL handle");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_rigpose_results: no run on the current inputs (pcs_rigpose_run first)");
    const auto out = rigpose_out_slots(p, pose, rms, info, hess, resid);
    return fetch_slots(p->core, out.data(), RIGPOSE_SLOTS, p->owned, p->n_groups != 0, "pcs_rigpose_results",
                       "the last run wrote some of these outputs to caller buffers (or computed no residuals)");
}

int pcs_rigpose_set_loss(pcs_rig_localiser *p, int kind, double f_scale) { return set_handle_loss("pcs_rigpose_set_loss", p ? &p->loss : nullptr, kind, f_scale); }

int pcs_rigpose_get_loss(pcs_rig_localiser *p, int *kind, double *f_scale) {
    return get_handle_loss("pcs_rigpose_get_loss", p ? &p->loss : nullptr, kind, f_scale);
}

int pcs_rigpose_costs(pcs_rig_localiser *p, double *cost) {
    if (!p || !cost) return fail(PCS_ERR_ARG, "pcs_rigpose_costs: bad arguments");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_rigpose_costs: no run on the current inputs (pcs_rigpose_run first)");
    return fetch_costs(p->core, p->cost, p->lin, cost, p->n_groups, "pcs_rigpose_costs");
}

int pcs_rigpose_last_kernel_ms(pcs_rig_localiser *p, float *kernel_ms) {
    return timer_ms("pcs_rigpose_last_kernel_ms", p ? &p->timer : nullptr, kernel_ms, "nothing has run yet");
}
}  // extern "C"
