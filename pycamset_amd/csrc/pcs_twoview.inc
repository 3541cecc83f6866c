// pcs_twoview.inc — host side of the two-view consensus (included by pcs_engine.hip; kernels: ba_twoview.hpp, ba_fivepoint.hpp).  Fence, buffers and output
// slots are those of pcs_handle.inc (DESIGN.md, "Batched handles").
extern "C" {
// ---- two-view relative pose (SURVEY f10): a handle that owns the camera table, the correspondence copies, the stage buffers and the outputs.
constexpr int TV_STAGES = 5;   // undistort, hypotheses, scores, selection, final
struct pcs_two_view {
    HandleCore core;
    hipEvent_t ev[TV_STAGES + 1] = {};   // one in front of every stage and one behind the last
    bool timed = false;
    int64_t n_cams = 0;
    bool have_cams = false;
    DevBuf tab;                               // camera table (TRI_CAM_STRIDE doubles per camera)
    DevBuf uva, uvb, start, pcams, cpair;     // handle-owned copies of the correspondences; cpair: the pair of every row
    int64_t n_corr = 0, n_pairs = -1;
    DevBuf order, hist;                       // pairs by row count (enqueue_group_order), built by the first run of a table
    bool order_valid = false;
    int n_hyp = 64;
    double inlier_px = 2.0;
    uint64_t seed = 0;
    int solver = TV_SOLVER_EIGHT_POINT, refine_iters = 0;   // pcs_twoview_set_solver
    DevBuf und, hyp_F, hyp_ok, score, sel, best;   // undistorted rows; per (pair, hypothesis) F, usable flag and score; per pair the selection
    DevBuf hyp_E, slot_T;                          // five-point solver: per slot (ten per hypothesis) E and the best of its four [R | t]
    DevBuf T, info, stats, flag;                   // handle-owned outputs
    int owned = 0;
    bool run_valid = false;
};

int pcs_twoview_create(pcs_two_view **out, int device, int64_t n_cams) {
    if (!out || n_cams < 2 || n_cams > INT32_MAX) return fail(PCS_ERR_ARG, "pcs_twoview_create: bad arguments (at least two cameras)");
    *out = nullptr;
    if (const int rc = open_device("pcs_twoview_create", device)) return rc;
    pcs_two_view *p = new pcs_two_view();
    p->n_cams = n_cams;
    hipError_t e = p->core.create(device);
    for (int i = 0; i <= TV_STAGES && e == hipSuccess; ++i) e = hipEventCreate(&p->ev[i]);
    if (e == hipSuccess) e = p->tab.alloc(n_cams * TRI_CAM_STRIDE, sizeof(double));
    if (e == hipSuccess) e = p->hist.alloc(GROUP_ORDER_HIST, sizeof(int32_t));
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_twoview_create: %s", hipGetErrorString(e));
        pcs_twoview_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_twoview_destroy(pcs_two_view *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->tab, &p->uva, &p->uvb, &p->start, &p->pcams, &p->cpair, &p->order, &p->hist, &p->und, &p->hyp_F, &p->hyp_ok, &p->score, &p->sel,
                     &p->best, &p->hyp_E, &p->slot_T, &p->T, &p->info, &p->stats, &p->flag},
                    {});
    for (hipEvent_t &e : p->ev)
        if (e) (void)hipEventDestroy(e);
    delete p;
    return PCS_OK;
}

int pcs_twoview_set_cameras(pcs_two_view *p, const double *intr) {
    if (!p || !intr) return fail(PCS_ERR_ARG, "pcs_twoview_set_cameras: bad arguments");
    std::vector<double> tab((size_t)p->n_cams * TRI_CAM_STRIDE, 0.0);
    for (int64_t c = 0; c < p->n_cams; ++c)
        for (int k = 0; k < 9; ++k) tab[c * TRI_CAM_STRIDE + 22 + k] = intr[9 * c + k];   // [fx cx fy cy k0 k1 p0 p1 k2]: the slab row as it is
    if (const int rc = set_fixed_array(p->core, p->tab, tab.data(), sizeof(double) * tab.size())) return rc;
    p->have_cams = true;
    p->run_valid = false;
    return PCS_OK;
}

// Everything is checked on the host before anything changes or the device is touched: a refused call keeps the previous table.
int pcs_twoview_set_correspondences(pcs_two_view *p, int64_t n_corr, const double *uv_a, const double *uv_b, int64_t n_pairs, const int64_t *start_inds,
                                    const int32_t *pair_cams) {
    const char *who = "pcs_twoview_set_correspondences";
    if (!p || n_corr < 0 || n_pairs < 0 || n_pairs > INT32_MAX || !start_inds || (n_corr > 0 && (!uv_a || !uv_b)) || (n_pairs > 0 && !pair_cams))
        return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (start_inds[0] != 0 || start_inds[n_pairs] != n_corr) return fail(PCS_ERR_ARG, "%s: start_inds must run from 0 to n_corr", who);
    for (int64_t j = 0; j < n_pairs; ++j) {
        if (start_inds[j + 1] < start_inds[j]) return fail(PCS_ERR_ARG, "%s: start_inds must be non-decreasing", who);
        const int32_t a = pair_cams[2 * j], b = pair_cams[2 * j + 1];
        if (const int rc = check_group_entity("pair", j, "camera a", a, p->n_cams)) return rc;
        if (const int rc = check_group_entity("pair", j, "camera b", b, p->n_cams)) return rc;
        if (a >= b) return fail(PCS_ERR_ARG, "%s: pair %lld has cameras (%d, %d), expected a < b", who, (long long)j, a, b);
    }
    for (int64_t r = 0; r < 2 * n_corr; ++r)
        if (!std::isfinite(uv_a[r]) || !std::isfinite(uv_b[r])) return fail(PCS_ERR_ARG, "%s: correspondence %lld has a non-finite pixel", who, (long long)(r / 2));
    std::vector<int32_t> cpair((size_t)n_corr);
    for (int64_t j = 0; j < n_pairs; ++j)
        for (int64_t r = start_inds[j]; r < start_inds[j + 1]; ++r) cpair[r] = (int32_t)j;
    HIPCHK(p->core.quiesce());
    p->n_pairs = -1;
    const HostArray arrays[] = {{p->uva, uv_a, n_corr, 2 * sizeof(double)}, {p->uvb, uv_b, n_corr, 2 * sizeof(double)},
                                {p->start, start_inds, n_pairs + 1, sizeof(int64_t)}, {p->pcams, pair_cams, n_pairs, 2 * sizeof(int32_t)},
                                {p->cpair, cpair.data(), n_corr, sizeof(int32_t)}};
    if (const int rc = upload_host_arrays(p->core, arrays, 5)) return rc;
    p->n_corr = n_corr;
    p->n_pairs = n_pairs;
    p->order_valid = false;
    p->run_valid = false;
    return PCS_OK;
}

static_assert(TV_OK == PCS_TWOVIEW_OK && TV_TOO_FEW == PCS_TWOVIEW_TOO_FEW && TV_DEGENERATE == PCS_TWOVIEW_DEGENERATE &&
              TV_NO_CHEIRALITY == PCS_TWOVIEW_NO_CHEIRALITY, "status codes of pcs_hip.h");
constexpr int TV_MAX_HYP = 256;
constexpr int64_t TV_WIDE_MEAN = 256;   // mean rows per pair from which a pair gets a whole wave (the width rule of rigpose_lm_kernel)

// cv2.findEssentialMat's RANSAC arguments.  Everything is checked before anything changes: a refused call keeps the previous setting.
int pcs_twoview_set_consensus(pcs_two_view *p, int n_hypotheses, double inlier_px, uint64_t seed) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_twoview_set_consensus: NULL handle");
    if (n_hypotheses < 1 || n_hypotheses > TV_MAX_HYP) return fail(PCS_ERR_RANGE, "pcs_twoview_set_consensus: n_hypotheses %d outside [1, %d]", n_hypotheses, TV_MAX_HYP);
    if (!std::isfinite(inlier_px) || !(inlier_px > 0.0)) return fail(PCS_ERR_ARG, "pcs_twoview_set_consensus: inlier_px must be finite and > 0 (got %g)", inlier_px);
    p->n_hyp = n_hypotheses;
    p->inlier_px = inlier_px;
    p->seed = seed;
    return PCS_OK;
}

int pcs_twoview_get_consensus(pcs_two_view *p, int *n_hypotheses, double *inlier_px, uint64_t *seed) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_twoview_get_consensus: NULL handle");
    if (n_hypotheses) *n_hypotheses = p->n_hyp;
    if (inlier_px) *inlier_px = p->inlier_px;
    if (seed) *seed = p->seed;
    return PCS_OK;
}

static_assert(TV_SOLVER_EIGHT_POINT == PCS_TWOVIEW_EIGHT_POINT && TV_SOLVER_FIVE_POINT == PCS_TWOVIEW_FIVE_POINT, "solver codes of pcs_hip.h");

// The hypothesis solver and the refinement behind the final model.  Everything is checked before anything changes: a refused call keeps
// the previous setting.
int pcs_twoview_set_solver(pcs_two_view *p, int solver, int refine_iters) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_twoview_set_solver: NULL handle");
    if (solver != TV_SOLVER_EIGHT_POINT && solver != TV_SOLVER_FIVE_POINT)
        return fail(PCS_ERR_ARG, "pcs_twoview_set_solver: solver %d is neither PCS_TWOVIEW_EIGHT_POINT nor PCS_TWOVIEW_FIVE_POINT", solver);
    if (refine_iters < 0 || refine_iters > TV_REFINE_MAX_ITERS)
        return fail(PCS_ERR_RANGE, "pcs_twoview_set_solver: refine_iters %d outside [0, %d]", refine_iters, TV_REFINE_MAX_ITERS);
    p->solver = solver;
    p->refine_iters = refine_iters;
    return PCS_OK;
}

int pcs_twoview_get_solver(pcs_two_view *p, int *solver, int *refine_iters) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_twoview_get_solver: NULL handle");
    if (solver) *solver = p->solver;
    if (refine_iters) *refine_iters = p->refine_iters;
    return PCS_OK;
}

enum { TV_SLOT_T, TV_SLOT_INFO, TV_SLOT_STATS, TV_SLOT_INLIER, TV_SLOTS };
static std::array<OutSlot, TV_SLOTS> tv_out_slots(pcs_two_view *p, void *o_T, void *o_info, void *o_stats, void *o_inlier) {
    const int64_t np = p->n_pairs;
    return {{{PCS_TWOVIEW_OUT_T, p->T, o_T, np, 12 * sizeof(double)}, {PCS_TWOVIEW_OUT_INFO, p->info, o_info, np, 5 * sizeof(int32_t)},
             {PCS_TWOVIEW_OUT_STATS, p->stats, o_stats, np, 3 * sizeof(double)}, {PCS_TWOVIEW_OUT_INLIER, p->flag, o_inlier, p->n_corr, sizeof(uint8_t)}}};
}

// The refinement behind either final kernel (it counts under "final"), the last event and the fence: the end of every run.
static int twoview_finish_run(pcs_two_view *p, OutSlot *out, int owned, bool wide, hipStream_t s) {
    if (p->refine_iters > 0) {
        const dim3 pair_g((unsigned)((p->n_pairs * (wide ? 64 : 16) + 255) / 256));
        const auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, pair_g, dim3(256), 0, s, p->und.as<const double4>(), p->start.as<const int64_t>(), p->pcams.as<const int32_t>(),
                               p->tab.as<const double>(), p->n_pairs, p->order.as<const int32_t>(), p->refine_iters, (const uint8_t *)out[TV_SLOT_INLIER].as<uint8_t>(),
                               out[TV_SLOT_T].as<double>(), out[TV_SLOT_INFO].as<int32_t>(), out[TV_SLOT_STATS].as<double>());
        };
        if (wide) launch(tv_refine_kernel<64>);
        else launch(tv_refine_kernel<16>);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->ev[5], s));
    p->timed = true;
    p->owned = owned;
    p->run_valid = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

// Stages 2 .. 5 of a run with the five-point solver (ba_fivepoint.hpp): ten candidate slots per hypothesis, scored with cheirality.
static int twoview_run_five_point(pcs_two_view *p, OutSlot *out, int owned, bool wide, int n_min, double tau2, hipStream_t s) {
    const int64_t np = p->n_pairs, H = p->n_hyp, nh = np * H, ns = nh * TV5_SLOTS;
    const int G = wide ? 64 : 16, HS = (int)(H * TV5_SLOTS);
    const double4 *und = p->und.as<const double4>();
    const int64_t *start = p->start.as<const int64_t>();
    const int32_t *pcams = p->pcams.as<const int32_t>(), *order = p->order.as<const int32_t>();
    const double *tab = p->tab.as<const double>();
    const dim3 hyp16((unsigned)((nh * 16 + 255) / 256)), slot_g((unsigned)((ns * G + 255) / 256)), pair_g((unsigned)((np * G + 255) / 256));
    hipLaunchKernelGGL(tv5_hypothesis_kernel, hyp16, dim3(256), 0, s, und, start, pcams, tab, np, (int)H, p->seed, p->hyp_E.as<double>(), p->hyp_F.as<double>(),
                       p->hyp_ok.as<uint8_t>());
    HIPCHK(hipEventRecord(p->ev[2], s));
    const double *hyp_E = p->hyp_E.as<const double>(), *hyp_F = p->hyp_F.as<const double>(), *score = p->score.as<const double>(), *slot_T = p->slot_T.as<const double>();
    uint8_t *flag = out[TV_SLOT_INLIER].as<uint8_t>();
    if (wide) hipLaunchKernelGGL((tv5_score_kernel<64>), slot_g, dim3(256), 0, s, und, start, pcams, tab, np, HS, hyp_E, hyp_F, p->hyp_ok.as<const uint8_t>(), tau2, p->score.as<double>(), p->slot_T.as<double>());
    else hipLaunchKernelGGL((tv5_score_kernel<16>), slot_g, dim3(256), 0, s, und, start, pcams, tab, np, HS, hyp_E, hyp_F, p->hyp_ok.as<const uint8_t>(), tau2, p->score.as<double>(), p->slot_T.as<double>());
    HIPCHK(hipEventRecord(p->ev[3], s));
    if (wide) hipLaunchKernelGGL((tv5_select_kernel<64>), pair_g, dim3(256), 0, s, und, start, pcams, tab, np, order, HS, n_min, hyp_F, slot_T, score, tau2, flag, p->sel.as<int32_t>(), p->best.as<double>());
    else hipLaunchKernelGGL((tv5_select_kernel<16>), pair_g, dim3(256), 0, s, und, start, pcams, tab, np, order, HS, n_min, hyp_F, slot_T, score, tau2, flag, p->sel.as<int32_t>(), p->best.as<double>());
    HIPCHK(hipEventRecord(p->ev[4], s));
    if (wide) hipLaunchKernelGGL((tv5_final_kernel<64>), pair_g, dim3(256), 0, s, und, start, pcams, tab, np, order, HS, n_min, (const uint8_t *)flag, p->sel.as<const int32_t>(),
                                 p->best.as<const double>(), slot_T, out[TV_SLOT_T].as<double>(), out[TV_SLOT_INFO].as<int32_t>(), out[TV_SLOT_STATS].as<double>());
    else hipLaunchKernelGGL((tv5_final_kernel<16>), pair_g, dim3(256), 0, s, und, start, pcams, tab, np, order, HS, n_min, (const uint8_t *)flag, p->sel.as<const int32_t>(),
                            p->best.as<const double>(), slot_T, out[TV_SLOT_T].as<double>(), out[TV_SLOT_INFO].as<int32_t>(), out[TV_SLOT_STATS].as<double>());
    return twoview_finish_run(p, out, owned, wide, s);
}

int pcs_twoview_run(pcs_two_view *p, int min_points, int group_lanes, int flags, double *d_T, void *stream) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_twoview_run: NULL handle");
    if (min_points < 1 || flags != 0 || (group_lanes != 0 && group_lanes != 16 && group_lanes != 64))
        return fail(PCS_ERR_ARG, "pcs_twoview_run: bad options (min_points >= 1, group_lanes 0, 16 or 64, no flags)");
    if (!p->have_cams || p->n_pairs < 0) return fail(PCS_ERR_STATE, "pcs_twoview_run: cameras or correspondences not set");
    auto out = tv_out_slots(p, d_T, nullptr, nullptr, nullptr);
    const bool five = p->solver == TV_SOLVER_FIVE_POINT;
    const int64_t np = p->n_pairs, H = p->n_hyp, nh = np * H, nc = std::max<int64_t>(1, p->n_corr);
    const int64_t ns = five ? nh * TV5_SLOTS : nh;   // scored candidates: ten slots per hypothesis of the five-point solver
    if (ns > INT32_MAX / 64) return fail(PCS_ERR_ARG, "pcs_twoview_run: %lld pairs x %lld hypotheses are more than one launch takes", (long long)np, (long long)H);
    struct Need { DevBuf &buf; int64_t count; size_t bytes; };
    const Need need[] = {{p->und, nc, 4 * sizeof(double)}, {p->hyp_F, ns, 9 * sizeof(double)}, {p->hyp_ok, ns, sizeof(uint8_t)}, {p->score, ns, sizeof(double)},
                         {p->sel, np, 2 * sizeof(int32_t)}, {p->best, np, sizeof(double)}, {p->order, np, sizeof(int32_t)},
                         {p->hyp_E, five ? ns : -1, 9 * sizeof(double)}, {p->slot_T, five ? ns : -1, 12 * sizeof(double)}};   // -1: not needed by this solver
    bool grows = false;
    for (const Need &n : need) grows = grows || (n.count >= 0 && n.buf.grows(std::max<int64_t>(1, n.count)));
    const int owned = owned_slots(out.data(), TV_SLOTS, &grows);
    if (np == 0) {
        p->owned = owned;
        p->run_valid = true;
        p->timed = false;   // nothing ran: no time of an earlier run is reported for this one
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));
    int rc = grow_owned_slots(out.data(), TV_SLOTS);
    for (const Need &n : need)
        if (!rc && n.count >= 0) rc = n.buf.grow(std::max<int64_t>(1, n.count), n.bytes);
    if (rc) return rc;
    if (!p->order_valid) {   // after every allocation: nothing is queued by a call that fails in one
        if ((rc = enqueue_group_order(p->start.as<int64_t>(), np, p->hist.as<int32_t>(), p->order.as<int32_t>(), s))) return rc;
        p->order_valid = true;
    }
    const bool wide = group_lanes == 64 || (group_lanes == 0 && p->n_corr >= TV_WIDE_MEAN * np);
    const int G = wide ? 64 : 16, n_min = std::max(five ? TV5_SAMPLE : TV_SAMPLE, min_points);
    const double tau2 = p->inlier_px * p->inlier_px;
    const double4 *und = p->und.as<const double4>();
    const int64_t *start = p->start.as<const int64_t>();
    const int32_t *pcams = p->pcams.as<const int32_t>(), *order = p->order.as<const int32_t>();
    const double *tab = p->tab.as<const double>();
    const dim3 hyp16((unsigned)((nh * 16 + 255) / 256)), hyp_g((unsigned)((nh * G + 255) / 256)), pair_g((unsigned)((np * G + 255) / 256));
    HIPCHK(hipEventRecord(p->ev[0], s));
    if (p->n_corr > 0)
        hipLaunchKernelGGL(tv_undistort_kernel, dim3((unsigned)((p->n_corr + 255) / 256)), dim3(256), 0, s, p->uva.as<const double2>(), p->uvb.as<const double2>(),
                           p->cpair.as<const int32_t>(), pcams, tab, p->n_corr, p->und.as<double4>());
    HIPCHK(hipEventRecord(p->ev[1], s));
    if (five) return twoview_run_five_point(p, out.data(), owned, wide, n_min, tau2, s);
    hipLaunchKernelGGL(tv_hypothesis_kernel, hyp16, dim3(256), 0, s, und, start, pcams, tab, np, (int)H, p->seed, p->hyp_F.as<double>(), p->hyp_ok.as<uint8_t>());
    HIPCHK(hipEventRecord(p->ev[2], s));
    const double *hyp_F = p->hyp_F.as<const double>(), *score = p->score.as<const double>();
    uint8_t *flag = out[TV_SLOT_INLIER].as<uint8_t>();
    if (wide) hipLaunchKernelGGL((tv_score_kernel<64>), hyp_g, dim3(256), 0, s, und, start, np, (int)H, hyp_F, p->hyp_ok.as<const uint8_t>(), tau2, p->score.as<double>());
    else hipLaunchKernelGGL((tv_score_kernel<16>), hyp_g, dim3(256), 0, s, und, start, np, (int)H, hyp_F, p->hyp_ok.as<const uint8_t>(), tau2, p->score.as<double>());
    HIPCHK(hipEventRecord(p->ev[3], s));
    if (wide) hipLaunchKernelGGL((tv_select_kernel<64>), pair_g, dim3(256), 0, s, und, start, np, order, (int)H, n_min, hyp_F, score, tau2, flag, p->sel.as<int32_t>(), p->best.as<double>());
    else hipLaunchKernelGGL((tv_select_kernel<16>), pair_g, dim3(256), 0, s, und, start, np, order, (int)H, n_min, hyp_F, score, tau2, flag, p->sel.as<int32_t>(), p->best.as<double>());
    HIPCHK(hipEventRecord(p->ev[4], s));
    if (wide) hipLaunchKernelGGL((tv_final_kernel<64>), pair_g, dim3(256), 0, s, und, start, pcams, tab, np, order, n_min, (const uint8_t *)flag, p->sel.as<const int32_t>(),
                                 p->best.as<const double>(), out[TV_SLOT_T].as<double>(), out[TV_SLOT_INFO].as<int32_t>(), out[TV_SLOT_STATS].as<double>());
    else hipLaunchKernelGGL((tv_final_kernel<16>), pair_g, dim3(256), 0, s, und, start, pcams, tab, np, order, n_min, (const uint8_t *)flag, p->sel.as<const int32_t>(),
                            p->best.as<const double>(), out[TV_SLOT_T].as<double>(), out[TV_SLOT_INFO].as<int32_t>(), out[TV_SLOT_STATS].as<double>());
    return twoview_finish_run(p, out.data(), owned, wide, s);
}

int pcs_twoview_results(pcs_two_view *p, double *T, int32_t *info, double *stats, uint8_t *inlier) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_twoview_results: NULL handle");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_twoview_results: no run on the current cameras and correspondences (pcs_twoview_run first)");
    const auto out = tv_out_slots(p, T, info, stats, inlier);
    return fetch_slots(p->core, out.data(), TV_SLOTS, p->owned, p->n_pairs != 0, "pcs_twoview_results", "the last run wrote T to a caller buffer");
}

// Device time of every stage of the last run: kernel_ms[0 .. 5) = undistort, hypotheses, scores, selection, final.
int pcs_twoview_last_kernel_ms(pcs_two_view *p, float *kernel_ms) {
    if (!p || !kernel_ms) return fail(PCS_ERR_ARG, "pcs_twoview_last_kernel_ms: bad arguments");
    if (!p->timed) return fail(PCS_ERR_STATE, "pcs_twoview_last_kernel_ms: nothing has run yet");
    HIPCHK(hipEventSynchronize(p->ev[TV_STAGES]));
    for (int i = 0; i < TV_STAGES; ++i) HIPCHK(hipEventElapsedTime(&kernel_ms[i], p->ev[i], p->ev[i + 1]));
    return PCS_OK;
}
}  // extern "C"
