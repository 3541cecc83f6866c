// pcs_align.inc — host side of the batched point-set registration (included by pcs_engine.hip; kernels: ba_align.hpp).  Fence, buffers and
// output slots are those of pcs_handle.inc (DESIGN.md, "Batched handles").
extern "C" {
// ---- rigid / similarity registration of 3-D point sets (SURVEY f11): a handle that owns the point table, the stage buffers and the outputs.
constexpr int ALIGN_STAGES = 4;   // hypotheses, scores, selection, fit
struct pcs_point_aligner {
    HandleCore core;
    hipEvent_t ev[ALIGN_STAGES + 1] = {};   // one in front of every stage and one behind the last
    bool timed = false;
    DevBuf src, dst, wt, start;             // handle-owned copies of the table
    bool have_wt = false;
    int64_t n_rows = 0, n_problems = -1;
    int n_hyp = 0;                          // 0: no consensus stage
    double inlier_dist = 0.0;
    uint64_t seed = 0;
    DevBuf hyp, score, sel, best;           // per (problem, hypothesis) [s R | t] and score; per problem the selection
    DevBuf T, scale, info, stats, flag, dist;   // handle-owned outputs
    int owned = 0;
    bool run_valid = false;
};

int pcs_align_create(pcs_point_aligner **out, int device) {
    if (!out) return fail(PCS_ERR_ARG, "pcs_align_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_align_create", device)) return rc;
    pcs_point_aligner *p = new pcs_point_aligner();
    hipError_t e = p->core.create(device);
    for (int i = 0; i <= ALIGN_STAGES && e == hipSuccess; ++i) e = hipEventCreate(&p->ev[i]);
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_align_create: %s", hipGetErrorString(e));
        pcs_align_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_align_destroy(pcs_point_aligner *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->src, &p->dst, &p->wt, &p->start, &p->hyp, &p->score, &p->sel, &p->best, &p->T, &p->scale, &p->info, &p->stats, &p->flag, &p->dist}, {});
    for (hipEvent_t &e : p->ev)
        if (e) (void)hipEventDestroy(e);
    delete p;
    return PCS_OK;
}

// Everything is checked on the host before anything changes or the device is touched: a refused call keeps the previous table.
// Non-finite COORDINATES are data (the row is skipped); a weight must be finite and >= 0.
int pcs_align_set_points(pcs_point_aligner *p, int64_t n_rows, const double *src, const double *dst, const double *weights, int64_t n_problems,
                         const int64_t *start_inds) {
    const char *who = "pcs_align_set_points";
    if (!p || n_rows < 0 || n_problems < 0 || n_problems > INT32_MAX || !start_inds || (n_rows > 0 && (!src || !dst))) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (start_inds[0] != 0 || start_inds[n_problems] != n_rows) return fail(PCS_ERR_ARG, "%s: start_inds must run from 0 to n_rows", who);
    for (int64_t j = 0; j < n_problems; ++j)
        if (start_inds[j + 1] < start_inds[j]) return fail(PCS_ERR_ARG, "%s: start_inds must be non-decreasing", who);
    if (weights)
        for (int64_t r = 0; r < n_rows; ++r)
            if (!std::isfinite(weights[r]) || !(weights[r] >= 0.0)) return fail(PCS_ERR_ARG, "%s: weight %lld = %g must be finite and >= 0", who, (long long)r, weights[r]);
    HIPCHK(p->core.quiesce());
    p->n_problems = -1;
    const HostArray arrays[] = {{p->src, src, n_rows, 3 * sizeof(double)}, {p->dst, dst, n_rows, 3 * sizeof(double)},
                                {p->start, start_inds, n_problems + 1, sizeof(int64_t)}, {p->wt, weights, weights ? n_rows : 0, sizeof(double)}};
    if (const int rc = upload_host_arrays(p->core, arrays, 4)) return rc;
    p->have_wt = weights != nullptr;
    p->n_rows = n_rows;
    p->n_problems = n_problems;
    p->run_valid = false;
    return PCS_OK;
}

static_assert(ALIGN_OK == PCS_ALIGN_OK && ALIGN_TOO_FEW == PCS_ALIGN_TOO_FEW && ALIGN_DEGENERATE == PCS_ALIGN_DEGENERATE && ALIGN_NONFINITE == PCS_ALIGN_NONFINITE &&
              ALIGN_NO_CONSENSUS == PCS_ALIGN_NO_CONSENSUS, "status codes of pcs_hip.h");
constexpr int ALIGN_MAX_HYP = 256;
constexpr int64_t ALIGN_WIDE_MEAN = 256;   // mean rows per problem from which a problem gets a whole wave (the width rule of rigpose_lm_kernel)

// The consensus stage in front of the fit, opt-in.  Everything is checked before anything changes: a refused call keeps the previous setting.
int pcs_align_set_consensus(pcs_point_aligner *p, int n_hypotheses, double inlier_dist, uint64_t seed) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_align_set_consensus: NULL handle");
    if (n_hypotheses < 0 || n_hypotheses > ALIGN_MAX_HYP) return fail(PCS_ERR_RANGE, "pcs_align_set_consensus: n_hypotheses %d outside [0, %d]", n_hypotheses, ALIGN_MAX_HYP);
    if (n_hypotheses > 0 && (!std::isfinite(inlier_dist) || !(inlier_dist > 0.0)))
        return fail(PCS_ERR_ARG, "pcs_align_set_consensus: inlier_dist must be finite and > 0 (got %g)", inlier_dist);
    p->n_hyp = n_hypotheses;
    p->inlier_dist = n_hypotheses > 0 ? inlier_dist : 0.0;
    p->seed = seed;
    return PCS_OK;
}

int pcs_align_get_consensus(pcs_point_aligner *p, int *n_hypotheses, double *inlier_dist, uint64_t *seed) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_align_get_consensus: NULL handle");
    if (n_hypotheses) *n_hypotheses = p->n_hyp;
    if (inlier_dist) *inlier_dist = p->inlier_dist;
    if (seed) *seed = p->seed;
    return PCS_OK;
}

enum { AL_SLOT_T, AL_SLOT_SCALE, AL_SLOT_INFO, AL_SLOT_STATS, AL_SLOT_INLIER, AL_SLOT_DIST, AL_SLOTS };
static std::array<OutSlot, AL_SLOTS> align_out_slots(pcs_point_aligner *p, void *o_T, void *o_scale, void *o_info, void *o_stats, void *o_inlier, void *o_dist) {
    const int64_t np = p->n_problems;
    return {{{PCS_ALIGN_OUT_T, p->T, o_T, np, 12 * sizeof(double)}, {PCS_ALIGN_OUT_SCALE, p->scale, o_scale, np, sizeof(double)},
             {PCS_ALIGN_OUT_INFO, p->info, o_info, np, 4 * sizeof(int32_t)}, {PCS_ALIGN_OUT_STATS, p->stats, o_stats, np, 3 * sizeof(double)},
             {PCS_ALIGN_OUT_INLIER, p->flag, o_inlier, p->n_rows, sizeof(uint8_t)}, {PCS_ALIGN_OUT_DIST, p->dist, o_dist, p->n_rows, sizeof(double)}}};
}

int pcs_align_run(pcs_point_aligner *p, int model, int min_points, double rank_tol, int group_lanes, int flags, double *d_T, void *stream) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_align_run: NULL handle");
    if ((model != PCS_ALIGN_RIGID && model != PCS_ALIGN_SIMILARITY) || min_points < ALIGN_SAMPLE || !(rank_tol >= 0.0 && rank_tol < 1.0) || flags != 0 ||
        (group_lanes != 0 && group_lanes != 16 && group_lanes != 64))
        return fail(PCS_ERR_ARG, "pcs_align_run: bad options (model PCS_ALIGN_RIGID or PCS_ALIGN_SIMILARITY, min_points >= 3, rank_tol in [0, 1), group_lanes 0, 16 or 64, no flags)");
    if (p->n_problems < 0) return fail(PCS_ERR_STATE, "pcs_align_run: points not set");
    auto out = align_out_slots(p, d_T, nullptr, nullptr, nullptr, nullptr, nullptr);
    const int64_t np = p->n_problems, H = p->n_hyp, nh = np * H;
    if (std::max(nh, np) > INT32_MAX / 64) return fail(PCS_ERR_ARG, "pcs_align_run: %lld problems x %lld hypotheses are more than one launch takes", (long long)np, (long long)H);
    struct Need { DevBuf &buf; int64_t count; size_t bytes; };
    const Need need[] = {{p->hyp, nh, 12 * sizeof(double)}, {p->score, nh, sizeof(double)}, {p->sel, H ? np : 0, 3 * sizeof(int32_t)}, {p->best, H ? np : 0, sizeof(double)}};
    bool grows = false;
    for (const Need &n : need) grows = grows || (n.count > 0 && n.buf.grows(n.count));
    const int owned = owned_slots(out.data(), AL_SLOTS, &grows);
    if (np == 0) {
        p->owned = owned;
        p->run_valid = true;
        p->timed = false;   // nothing ran: no time of an earlier run is reported for this one
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));
    int rc = grow_owned_slots(out.data(), AL_SLOTS);
    for (const Need &n : need)
        if (!rc && n.count > 0) rc = n.buf.grow(n.count, n.bytes);
    if (rc) return rc;
    const bool wide = group_lanes == 64 || (group_lanes == 0 && p->n_rows >= ALIGN_WIDE_MEAN * np);
    const int G = wide ? 64 : 16;
    const double tau2 = p->inlier_dist * p->inlier_dist;
    const double *src = p->src.as<const double>(), *dst = p->dst.as<const double>(), *wt = p->have_wt ? p->wt.as<const double>() : nullptr;
    const int64_t *start = p->start.as<const int64_t>();
    uint8_t *flag = out[AL_SLOT_INLIER].as<uint8_t>();
    const dim3 hyp_t((unsigned)((nh + 255) / 256)), hyp_g((unsigned)((nh * G + 255) / 256)), prob_g((unsigned)((np * G + 255) / 256));
    HIPCHK(hipEventRecord(p->ev[0], s));
    if (H > 0) hipLaunchKernelGGL(align_hypothesis_kernel, hyp_t, dim3(256), 0, s, src, dst, wt, start, np, (int)H, p->seed, model, rank_tol, p->hyp.as<double>());
    HIPCHK(hipEventRecord(p->ev[1], s));
    if (H > 0) {
        if (wide) hipLaunchKernelGGL((align_score_kernel<64>), hyp_g, dim3(256), 0, s, src, dst, wt, start, np, (int)H, p->hyp.as<const double>(), tau2, p->score.as<double>());
        else hipLaunchKernelGGL((align_score_kernel<16>), hyp_g, dim3(256), 0, s, src, dst, wt, start, np, (int)H, p->hyp.as<const double>(), tau2, p->score.as<double>());
    }
    HIPCHK(hipEventRecord(p->ev[2], s));
    if (H > 0) {
        if (wide) hipLaunchKernelGGL((align_select_kernel<64>), prob_g, dim3(256), 0, s, src, dst, wt, start, np, (int)H, p->hyp.as<const double>(), p->score.as<const double>(), tau2, flag, p->sel.as<int32_t>(), p->best.as<double>());
        else hipLaunchKernelGGL((align_select_kernel<16>), prob_g, dim3(256), 0, s, src, dst, wt, start, np, (int)H, p->hyp.as<const double>(), p->score.as<const double>(), tau2, flag, p->sel.as<int32_t>(), p->best.as<double>());
    }
    HIPCHK(hipEventRecord(p->ev[3], s));
    // the fit: on the flags of the selection, or on every row (and then it writes the flags itself)
    const uint8_t *mask = H > 0 ? flag : nullptr;
    uint8_t *flag_out = H > 0 ? nullptr : flag;
    const int32_t *sel = H > 0 ? p->sel.as<const int32_t>() : nullptr;
    const double *best = H > 0 ? p->best.as<const double>() : nullptr;
    if (wide) hipLaunchKernelGGL((align_fit_kernel<64>), prob_g, dim3(256), 0, s, src, dst, wt, start, np, model, min_points, rank_tol, mask, sel, best, out[AL_SLOT_T].as<double>(),
                                 out[AL_SLOT_SCALE].as<double>(), out[AL_SLOT_INFO].as<int32_t>(), out[AL_SLOT_STATS].as<double>(), flag_out, out[AL_SLOT_DIST].as<double>());
    else hipLaunchKernelGGL((align_fit_kernel<16>), prob_g, dim3(256), 0, s, src, dst, wt, start, np, model, min_points, rank_tol, mask, sel, best, out[AL_SLOT_T].as<double>(),
                            out[AL_SLOT_SCALE].as<double>(), out[AL_SLOT_INFO].as<int32_t>(), out[AL_SLOT_STATS].as<double>(), flag_out, out[AL_SLOT_DIST].as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->ev[4], s));
    p->timed = true;
    p->owned = owned;
    p->run_valid = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_align_results(pcs_point_aligner *p, double *T, double *scale, int32_t *info, double *stats, uint8_t *inlier, double *dist) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_align_results: NULL handle");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_align_results: no run on the current points (pcs_align_run first)");
    const auto out = align_out_slots(p, T, scale, info, stats, inlier, dist);
    return fetch_slots(p->core, out.data(), AL_SLOTS, p->owned, p->n_problems != 0, "pcs_align_results", "the last run wrote T to a caller buffer");
}

// Device time of every stage of the last run: kernel_ms[0 .. 4) = hypotheses, scores, selection, fit (the first three 0 without consensus).
int pcs_align_last_kernel_ms(pcs_point_aligner *p, float *kernel_ms) {
    if (!p || !kernel_ms) return fail(PCS_ERR_ARG, "pcs_align_last_kernel_ms: bad arguments");
    if (!p->timed) return fail(PCS_ERR_STATE, "pcs_align_last_kernel_ms: nothing has run yet");
    HIPCHK(hipEventSynchronize(p->ev[ALIGN_STAGES]));
    for (int i = 0; i < ALIGN_STAGES; ++i) HIPCHK(hipEventElapsedTime(&kernel_ms[i], p->ev[i], p->ev[i + 1]));
    return PCS_OK;
}
}  // extern "C"
