// pcs_triangulator.inc — host side of the batched triangulation (included by pcs_engine.hip; kernels: ba_triangulate.hpp, ba_tri_refine.hpp,
// ba_tri_consensus.hpp).
// Fence, buffers and output slots are those of pcs_handle.inc (DESIGN.md, "Batched handles").
extern "C" {
// ---- batched triangulation (SURVEY f4): a handle that owns the camera table, the observation buffers and the
// kernel's scratch, so that repeated calls (CameraSet.multi_cam_triangulate per frame set, cameras/camera_set.py:343-402)
// pay neither allocations nor — with device-resident inputs — copies.
struct pcs_triangulator {
    HandleCore core;
    KernelTimer timer, refine_timer;
    int64_t n_cams = 0;
    bool have_cams = false;
    DevBuf tab;                // camera table
    DevBuf cam, uv, start;     // handle-owned copies of host inputs (grown on demand)
    DevBuf scr, scl, pts;      // scratch (Householder row r_i; (1 / E_i, lambda_i) per observation) + default output
    // current problem (device pointers: handle-owned or the caller's)
    const int32_t *cur_cam = nullptr; const double *cur_uv = nullptr; const int64_t *cur_start = nullptr;
    int64_t n_obs = 0, n_pts = -1;
    DevBuf count, block_sums, totals;   // the grouping in front of the triangulation (pcs_tri_group_device): per-feature counts, block sums of the scan, totals
    DevBuf order, hist;                 // points by view count (enqueue_group_order), built by the first run of a set of observations
    bool order_valid = false, sort_points = true;
    int variant = 1; // 1: views in registers + divide-free rotations (round 4; 3: eight instead of six register views per lane); 0: round 3's kernel (PCS_TRI_VARIANT=0)
    int lanes = 4;   // lanes per point: 1, 2, 4, 8 or 16 (profiles/r01/tri_legacy_bench.log: 4 is fastest at 2-22 views)
    bool out_owned = false;   // the last run wrote the handle-owned output (pcs_tri_points has something to return)
    // the refinement (pcs_tri_refine): it starts from the points of the last run on the current cameras and observations
    bool run_valid = false;          // a run since the cameras / observations were last set
    const double *run_pts = nullptr; // where that run wrote its points (handle-owned or the caller's buffer)
    DevBuf rpts, rrms, rres, rinfo;  // handle-owned refinement outputs
    DevBuf rcost;                    // (n_pts, 2) 0.5 sum rho0 at the point and at the DLT point of the last refinement: always handle-owned
    LinearCosts rlin;                // a linear refinement derives them in pcs_tri_refine_costs
    HandleLoss refine_loss;          // pcs_tri_set_refine_loss: the handle's, whatever cameras and observations follow
    int refine_owned = 0;            // PCS_TRI_OUT_* bits: which outputs of the last refinement are handle-owned
    bool refine_valid = false;       // a refinement since the last run (pcs_tri_refined has something to return)
    // the consensus stage (pcs_tri_set_consensus; kernels: ba_tri_consensus.hpp).  cons_hyp = 0: off, and none of these buffers exists.
    int cons_hyp = 0;
    double cons_px = 8.0;
    uint64_t cons_seed = 0;
    bool cons_ran = false;                         // the last run had the stage: it and its refinement work on the compacted table
    DevBuf s_cam, s_uv, s_start, h_pts;            // the pseudo-points of the sampled pairs and their hypotheses
    DevBuf score, flag, cinfo, best;               // (n_pts, H) scores; per observation flag; per point record and winning score
    DevBuf c_cam, c_uv, c_start, c_order;          // the table compacted to inliers and its visiting order
};

int pcs_tri_create(pcs_triangulator **out, int device, int64_t n_cams) {
    if (!out || n_cams <= 0) return fail(PCS_ERR_ARG, "pcs_tri_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_tri_create", device)) return rc;
    pcs_triangulator *t = new pcs_triangulator();
    t->n_cams = n_cams;
    const char *lanes_env = getenv("PCS_TRI_LANES");   // A/B switch
    const int lanes = lanes_env ? atoi(lanes_env) : 4;
    t->lanes = (lanes == 1 || lanes == 2 || lanes == 8 || lanes == 16) ? lanes : 4;
    const char *var_env = getenv("PCS_TRI_VARIANT");
    t->variant = var_env ? atoi(var_env) : 1;
    t->sort_points = getenv("PCS_TRI_NO_SORT") == nullptr;   // A/B switch
    hipError_t e = t->core.create(device);
    if (e == hipSuccess) e = t->timer.create();
    if (e == hipSuccess) e = t->refine_timer.create();
    if (e == hipSuccess) e = t->tab.alloc(n_cams * TRI_CAM_STRIDE, sizeof(double));
    if (e == hipSuccess) e = t->hist.alloc(GROUP_ORDER_HIST, sizeof(int32_t));
    if (e == hipSuccess) e = t->totals.alloc(4, sizeof(int64_t));
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_tri_create: %s", hipGetErrorString(e));
        pcs_tri_destroy(t);
        return rc;
    }
    *out = t;
    return PCS_OK;
}

// what pcs_tri_run launches for this handle — the one place that turns the switches read at creation into a kernel geometry
struct TriLaunch {
    int lanes, reg_views;   // G; V (0: the scratch kernel)
    bool sorted;            // the points are visited in order of their view count
};
static TriLaunch tri_launch(const pcs_triangulator *t) {
    if (t->variant == 0) return {t->lanes, 0, false};
    return {t->lanes, t->lanes == 4 && t->variant != 3 ? 6 : 8, t->sort_points};
}

int pcs_tri_launch_config(pcs_triangulator *t, int32_t out[4]) {
    if (!t || !out) return fail(PCS_ERR_ARG, "pcs_tri_launch_config: bad arguments");
    const TriLaunch l = tri_launch(t);
    out[0] = l.lanes;
    out[1] = l.reg_views;
    out[2] = l.reg_views != 0;
    out[3] = l.sorted;
    return PCS_OK;
}

int pcs_tri_destroy(pcs_triangulator *t) {
    if (!t) return PCS_OK;
    t->core.destroy({&t->tab, &t->cam, &t->uv, &t->start, &t->scr, &t->scl, &t->pts, &t->count, &t->block_sums, &t->totals, &t->order, &t->hist, &t->rpts,
                     &t->rrms, &t->rres, &t->rinfo, &t->rcost, &t->s_cam, &t->s_uv, &t->s_start, &t->h_pts, &t->score, &t->flag, &t->cinfo, &t->best,
                     &t->c_cam, &t->c_uv, &t->c_start, &t->c_order},
                    {&t->timer, &t->refine_timer});
    delete t;
    return PCS_OK;
}

// a new set of observations (handle-owned copies or the caller's device arrays): results of an earlier problem are not this problem's,
// and a refinement must start from points of these observations
static void tri_new_problem(pcs_triangulator *t, const int32_t *d_cam, const double *d_uv, const int64_t *d_start, int64_t n_obs, int64_t n_pts) {
    t->cur_cam = d_cam; t->cur_uv = d_uv; t->cur_start = d_start;
    t->n_obs = n_obs; t->n_pts = n_pts;
    t->order_valid = false;
    t->out_owned = false;
    t->run_valid = t->refine_valid = false;
}
static void tri_own_problem(pcs_triangulator *t, int64_t n_obs, int64_t n_pts) {
    tri_new_problem(t, t->cam.as<int32_t>(), t->uv.as<double>(), t->start.as<int64_t>(), n_obs, n_pts);
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
    HIPCHK(t->core.quiesce());
    HIPCHK(hipMemcpy(t->tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
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
    HIPCHK(t->core.quiesce());
    t->n_pts = -1;
    const HostArray arrays[] = {{t->cam, cam, n_obs, sizeof(int32_t)}, {t->uv, uv, n_obs, 2 * sizeof(double)}, {t->start, start_inds, n_pts + 1, sizeof(int64_t)}};
    if (const int rc = upload_host_arrays(t->core, arrays, 3)) return rc;
    tri_own_problem(t, n_obs, n_pts);
    return PCS_OK;
}

int pcs_tri_set_observations_device(pcs_triangulator *t, int64_t n_obs, const int32_t *d_cam, const double *d_uv, int64_t n_pts, const int64_t *d_start_inds) {
    if (!t || n_obs < 0 || n_pts < 0 || !d_start_inds || (n_obs > 0 && (!d_cam || !d_uv))) return fail(PCS_ERR_ARG, "pcs_tri_set_observations_device: bad arguments");
    tri_new_problem(t, d_cam, d_uv, d_start_inds, n_obs, n_pts);   // caller-owned, not range-checked (stay on the device)
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
    hipStream_t s = t->core.stream_or(stream);
    HIPCHK(t->core.quiesce());   // a run queued on ANY stream may still read the observation copies this call overwrites
    t->n_pts = -1;
    t->run_valid = t->refine_valid = false;
    int rc;
    if (n == 0) {
        if ((rc = t->start.grow(1, sizeof(int64_t)))) return rc;
        HIPCHK(hipMemsetAsync(t->start.p, 0, sizeof(int64_t), s));
        HIPCHK(hipStreamSynchronize(s));
        tri_own_problem(t, 0, 0);
        return PCS_OK;
    }
    const int64_t n_blocks = (n + TRI_GROUP_BLOCK - 1) / TRI_GROUP_BLOCK;
    if ((rc = t->cam.grow(n, sizeof(int32_t)))) return rc;
    if ((rc = t->uv.grow(n, 2 * sizeof(double)))) return rc;
    // one entry per kept run + 1.  A GROUPED table has at most n / 2 kept runs, but whether it is grouped is only known afterwards: in a table
    // whose features interleave every row can be the head of a kept run (writes up to start[n]; sized for n / 2 + 2 until this was found
    // by a fault in the full test suite — alone, the overrun stayed inside the allocation)
    if ((rc = t->start.grow(n + 2, sizeof(int64_t)))) return rc;
    if ((rc = t->count.grow(n_features, sizeof(int32_t)))) return rc;
    if ((rc = t->block_sums.grow(n_blocks, sizeof(uint64_t)))) return rc;
    HIPCHK(hipMemsetAsync(t->count.p, 0, sizeof(int32_t) * n_features, s));
    HIPCHK(hipMemsetAsync(t->totals.p, 0, sizeof(int64_t) * 4, s));
    TriGroupArgs a{d_cam, d_feat, reinterpret_cast<const double2 *>(d_uv), t->count.as<int32_t>(), t->block_sums.as<uint64_t>(), t->totals.as<int64_t>(),
                   t->cam.as<int32_t>(), t->uv.as<double2>(), t->start.as<int64_t>(), n, n_features, (int32_t)n_blocks};
    hipLaunchKernelGGL(tri_group_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tri_group_blocksum_kernel, dim3((unsigned)n_blocks), dim3(TRI_GROUP_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tri_group_scan_sums_kernel, dim3(1), dim3(TRI_GROUP_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tri_group_scatter_kernel, dim3((unsigned)n_blocks), dim3(TRI_GROUP_BLOCK), 0, s, a);
    HIPCHK(hipGetLastError());
    int64_t totals[4];
    HIPCHK(hipMemcpyAsync(totals, t->totals.p, sizeof totals, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (totals[2] != totals[3]) {   // more runs than features: some feature's rows are not consecutive
        *grouped = 0;
        return PCS_OK;
    }
    *n_kept = totals[0];
    *n_pts = totals[1];
    tri_own_problem(t, totals[0], totals[1]);
    return PCS_OK;
}

// One launch of the triangulation kernel that tri_launch names, on any table: the handle's observations, the pseudo-points of the
// consensus stage, the table compacted to inliers.  e0 / e1: the events of hipExtLaunchKernelGGL around the kernel, or NULL.
static void tri_launch_dlt(pcs_triangulator *t, const TriLaunch &launch, hipStream_t s, hipEvent_t e0, hipEvent_t e1, const int32_t *cam, const double *uv,
                           const int64_t *start, double *d_pts, int64_t n_pts, const int32_t *order) {
    const int lanes = launch.lanes;
    const dim3 grid((unsigned)((n_pts * lanes + 255) / 256));
#define PCS_TRI_LAUNCH(G_)                                                                                                                       \
    hipExtLaunchKernelGGL(triangulate_kernel<G_>, grid, dim3(256), 0, s, e0, e1, 0, cam, (const double2 *)uv, start, t->tab.as<const double>(), \
                          t->scr.as<double4>(), t->scl.as<double2>(), d_pts, n_pts)
#define PCS_TRI_LAUNCH_REG(G_, V_)                                                                                                                       \
    hipExtLaunchKernelGGL((triangulate_reg_kernel<G_, V_>), grid, dim3(256), 0, s, e0, e1, 0, cam, (const double2 *)uv, start, t->tab.as<const double>(), \
                          t->scr.as<double4>(), t->scl.as<double2>(), d_pts, n_pts, order)
    if (launch.reg_views == 0) {   // round 3's form (views in the global scratch, IEEE divides): kept for A/B (PCS_TRI_VARIANT=0)
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
        else if (launch.reg_views == 8) PCS_TRI_LAUNCH_REG(4, 8);
        else PCS_TRI_LAUNCH_REG(4, 6);   // 24 views in registers at 156 VGPRs (three waves per SIMD): 47 us against 52 us for (4, 8); (4, 3) — four waves
                                         // per SIMD, 12 register views, the rest through the scratch records — 53 us, (4, 4) 49 us (profiles/r05/tri_bench_r05.log)
    }
#undef PCS_TRI_LAUNCH_REG
#undef PCS_TRI_LAUNCH
}

constexpr int TRI_CONS_MAX_HYP = 256;   // hypotheses per point that pcs_tri_set_consensus takes
constexpr int TRI_CONS_G = 4;           // lanes per point and per (point, hypothesis) of the stage: the DLT kernel's default

// The stage in front of the DLT (the two-view RANSAC in front of an n-view triangulation).  Everything is checked before anything
// changes: a refused call keeps the previous setting.
int pcs_tri_set_consensus(pcs_triangulator *t, int n_hypotheses, double inlier_px, uint64_t seed) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_set_consensus: NULL handle");
    if (n_hypotheses < 0 || n_hypotheses > TRI_CONS_MAX_HYP || !std::isfinite(inlier_px) || !(inlier_px > 0.0))
        return fail(PCS_ERR_ARG, "pcs_tri_set_consensus: bad arguments (0 <= n_hypotheses <= %d, inlier_px finite and > 0)", TRI_CONS_MAX_HYP);
    t->cons_hyp = n_hypotheses;
    t->cons_px = inlier_px;
    t->cons_seed = seed;
    return PCS_OK;
}

int pcs_tri_get_consensus(pcs_triangulator *t, int *n_hypotheses, double *inlier_px, uint64_t *seed) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_get_consensus: NULL handle");
    if (n_hypotheses) *n_hypotheses = t->cons_hyp;
    if (inlier_px) *inlier_px = t->cons_px;
    if (seed) *seed = t->cons_seed;
    return PCS_OK;
}

// A run with the consensus stage: used counts and their scan, sample, hypotheses by the handle's unchanged triangulation kernel on the
// pseudo-points, score, select, scan, compact; then the order and the DLT, unchanged, on the compacted table.  No host synchronisation:
// the compacted table is never longer than the handle's, so nothing on the host needs its total.
static int tri_run_consensus(pcs_triangulator *t, double *d_pts, void *stream) {
    const TriLaunch launch = tri_launch(t);
    const int64_t np = t->n_pts, H = t->cons_hyp, nh = np * H, no = std::max<int64_t>(1, t->n_obs);
    if (np > 0 && nh > ((int64_t)INT32_MAX * 256) / 16)
        return fail(PCS_ERR_ARG, "pcs_tri_run: %lld points x %lld hypotheses are more than one launch takes", (long long)np, (long long)H);
    const bool sorted = launch.sorted && np < (1ll << 31);
    // the scratch kernel keeps a record per observation, pseudo-points included; the register kernels hold two views in registers
    const int64_t scr_need = launch.reg_views == 0 ? std::max<int64_t>(no, 2 * nh) : no;
    struct Need { DevBuf &buf; int64_t count; size_t bytes; };
    const Need need[] = {{t->scr, scr_need, 4 * sizeof(double)}, {t->scl, scr_need, 2 * sizeof(double)},
                         {t->s_cam, 2 * nh, sizeof(int32_t)}, {t->s_uv, 2 * nh, 2 * sizeof(double)}, {t->s_start, nh + 1, sizeof(int64_t)},
                         {t->h_pts, nh, 3 * sizeof(double)}, {t->score, nh, sizeof(double)}, {t->flag, no, sizeof(uint8_t)},
                         {t->cinfo, np, 4 * sizeof(int32_t)}, {t->best, np, sizeof(double)}, {t->c_cam, no, sizeof(int32_t)},
                         {t->c_uv, no, 2 * sizeof(double)}, {t->c_start, np + 1, sizeof(int64_t)}, {t->c_order, sorted ? np : 1, sizeof(int32_t)}};
    OutSlot out{1, t->pts, d_pts, np, 3 * sizeof(double)};
    bool grows = false;
    for (const Need &n : need) grows = grows || n.buf.grows(std::max<int64_t>(1, n.count));
    const bool owned = owned_slots(&out, 1, &grows);
    if (np == 0) {
        t->run_valid = true;
        t->run_pts = d_pts;
        t->cons_ran = true;
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(t->core.device));
    hipStream_t s = t->core.stream_or(stream);
    HIPCHK(t->core.fence.before_run(s, grows));
    int rc = grow_owned_slots(&out, 1);
    for (const Need &n : need)
        if (!rc) rc = n.buf.grow(std::max<int64_t>(1, n.count), n.bytes);
    if (rc) return rc;
    d_pts = out.as<double>();
    HIPCHK(hipEventRecord(t->timer.e0, s));   // after every allocation: nothing is queued by a call that fails in one
    const int32_t *cam = t->cur_cam;
    const double2 *uv = (const double2 *)t->cur_uv;
    const int64_t *start = t->cur_start;
    const double *tab = t->tab.as<const double>();
    const double tau2 = t->cons_px * t->cons_px;
    constexpr int G = TRI_CONS_G;
    const dim3 per_pt((unsigned)((np + 255) / 256)), pt_groups((unsigned)((np * G + 255) / 256)), hyp_groups((unsigned)((nh * G + 255) / 256));
    // c_start first holds the row bases of the pseudo-table (the scan of the used counts), then the starts of the compacted table
    hipLaunchKernelGGL(tri_cons_used_kernel, per_pt, dim3(256), 0, s, start, np, (int)H, t->cinfo.as<int32_t>());
    hipLaunchKernelGGL(cons_count_scan_kernel, dim3(1), dim3(CONS_SCAN_THREADS), 0, s, t->cinfo.as<const int32_t>(), np, t->c_start.as<int64_t>());
    hipLaunchKernelGGL(tri_sample_kernel, dim3((unsigned)((nh + 255) / 256)), dim3(256), 0, s, cam, uv, start, t->c_start.as<const int64_t>(), np, (int)H,
                       t->cons_seed, t->s_cam.as<int32_t>(), t->s_uv.as<double2>(), t->s_start.as<int64_t>());
    tri_launch_dlt(t, launch, s, nullptr, nullptr, t->s_cam.as<const int32_t>(), t->s_uv.as<const double>(), t->s_start.as<const int64_t>(),
                   t->h_pts.as<double>(), nh, nullptr);
    hipLaunchKernelGGL((tri_score_kernel<G, false>), hyp_groups, dim3(256), 0, s, cam, uv, start, tab, np, (int)H, t->h_pts.as<const double>(), tau2,
                       t->score.as<double>(), (double *)nullptr);
    hipLaunchKernelGGL((tri_select_kernel<G>), pt_groups, dim3(256), 0, s, cam, uv, start, tab, np, (int)H, t->h_pts.as<const double>(),
                       t->score.as<const double>(), tau2, t->flag.as<uint8_t>(), t->cinfo.as<int32_t>(), t->best.as<double>());
    enqueue_compact_flagged<G>(cam, uv, start, t->flag.as<const uint8_t>(), t->cinfo.as<const int32_t>(), np, t->c_start.as<int64_t>(), t->c_cam.as<int32_t>(),
                               t->c_uv.as<double2>(), s);
    HIPCHK(hipGetLastError());
    if (sorted)
        if ((rc = enqueue_group_order(t->c_start.as<int64_t>(), np, t->hist.as<int32_t>(), t->c_order.as<int32_t>(), s))) return rc;
    tri_launch_dlt(t, launch, s, nullptr, nullptr, t->c_cam.as<const int32_t>(), t->c_uv.as<const double>(), t->c_start.as<const int64_t>(), d_pts, np,
                   sorted ? t->c_order.as<const int32_t>() : nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(t->timer.e1, s));
    t->timer.timed = true;
    t->out_owned = owned;
    t->run_valid = true;
    t->run_pts = d_pts;
    t->cons_ran = true;
    HIPCHK(t->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_tri_run(pcs_triangulator *t, double *d_pts, void *stream) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_run: bad arguments");
    if (!t->have_cams) return fail(PCS_ERR_STATE, "pcs_tri_run: cameras not set");
    if (t->n_pts < 0) return fail(PCS_ERR_STATE, "pcs_tri_run: observations not set");
    t->refine_valid = false;
    if (t->cons_hyp > 0) return tri_run_consensus(t, d_pts, stream);
    t->cons_ran = false;
    if (t->n_pts == 0) {
        t->run_valid = true;
        t->run_pts = d_pts;
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(t->core.device));
    hipStream_t s = t->core.stream_or(stream);
    const TriLaunch launch = tri_launch(t);
    const bool need_order = launch.sorted && !t->order_valid && t->n_pts < (1ll << 31);
    const int64_t obs_alloc = std::max<int64_t>(1, t->n_obs);
    OutSlot out{1, t->pts, d_pts, t->n_pts, 3 * sizeof(double)};
    bool grows = t->scr.grows(t->n_obs) || t->scl.grows(t->n_obs) || (need_order && t->order.grows(t->n_pts));
    const bool owned = owned_slots(&out, 1, &grows);
    HIPCHK(t->core.fence.before_run(s, grows));   // scratch and output are shared between runs
    int rc = t->scr.grow(obs_alloc, 4 * sizeof(double));
    if (!rc) rc = t->scl.grow(obs_alloc, 2 * sizeof(double));
    if (!rc) rc = grow_owned_slots(&out, 1);
    if (!rc && need_order) rc = t->order.grow(t->n_pts, sizeof(int32_t));
    if (rc) return rc;
    d_pts = out.as<double>();
    if (need_order) {
        if ((rc = enqueue_group_order(t->cur_start, t->n_pts, t->hist.as<int32_t>(), t->order.as<int32_t>(), s))) return rc;
        t->order_valid = true;
    }
    tri_launch_dlt(t, launch, s, t->timer.e0, t->timer.e1, t->cur_cam, t->cur_uv, t->cur_start, d_pts, t->n_pts,
                   t->order_valid ? t->order.as<const int32_t>() : nullptr);
    HIPCHK(hipGetLastError());
    t->timer.timed = true;
    t->out_owned = owned;
    t->run_valid = true;
    t->run_pts = d_pts;
    HIPCHK(t->core.fence.after_run(s));
    return PCS_OK;
}

// The refinement of the last run's points (csrc/ba_tri_refine.hpp): per-point LM on the reprojection error in the measured pixels.
static_assert(TRI_REFINE_NOT_REFINED == PCS_TRI_REFINE_NOT_REFINED && TRI_REFINE_CONVERGED == PCS_TRI_REFINE_CONVERGED &&
              TRI_REFINE_MAX_ITER == PCS_TRI_REFINE_MAX_ITER && TRI_REFINE_NO_DECREASE == PCS_TRI_REFINE_NO_DECREASE, "status codes of pcs_hip.h");

// the outputs in the order of the PCS_TRI_OUT_* bits; the residuals last, so that a refinement without them takes the first three
enum { TRI_SLOT_POINTS, TRI_SLOT_RMS, TRI_SLOT_INFO, TRI_SLOT_RESID, TRI_SLOTS };
static std::array<OutSlot, TRI_SLOTS> tri_out_slots(pcs_triangulator *t, void *o_pts, void *o_rms, void *o_info, void *o_resid) {
    const int64_t n = t->n_pts;
    return {{{PCS_TRI_OUT_POINTS, t->rpts, o_pts, n, 3 * sizeof(double)}, {PCS_TRI_OUT_RMS, t->rrms, o_rms, n, 2 * sizeof(double)},
             {PCS_TRI_OUT_INFO, t->rinfo, o_info, n, 3 * sizeof(int32_t)}, {PCS_TRI_OUT_RESIDUALS, t->rres, o_resid, t->n_obs, 2 * sizeof(double)}}};
}

int pcs_tri_refine(pcs_triangulator *t, int max_iter, double ftol, double xtol, double gtol, int flags, double *d_pts, double *d_rms,
                   int32_t *d_info, double *d_resid, void *stream) {
    const bool rest_ok = !(flags & ~PCS_TRI_REFINE_RESIDUALS);
    if (const int rc = check_lm_options("pcs_tri_refine", max_iter, ftol, xtol, gtol, rest_ok, "flags PCS_TRI_REFINE_RESIDUALS")) return rc;
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_refine: NULL handle");
    if (!t->have_cams || t->n_pts < 0 || !t->run_valid)
        return fail(PCS_ERR_STATE, "pcs_tri_refine: no run on the current cameras and observations (pcs_tri_run first)");
    const bool want_resid = flags & PCS_TRI_REFINE_RESIDUALS;
    auto out = tri_out_slots(t, d_pts, d_rms, d_info, d_resid);
    const int n_out = want_resid ? TRI_SLOTS : TRI_SLOTS - 1;
    const bool robust = t->refine_loss.kind != PCS_LOSS_LINEAR;
    bool grows = robust && t->rcost.grows(t->n_pts);
    const int owned = owned_slots(out.data(), n_out, &grows);
    if (t->n_pts == 0) {
        t->rlin.pending = false;
        t->refine_owned = owned;
        t->refine_valid = true;
        return PCS_OK;
    }
    HIPCHK(hipSetDevice(t->core.device));
    hipStream_t s = t->core.stream_or(stream);
    HIPCHK(t->core.fence.before_run(s, grows));   // the run (or an earlier refinement) first: this reads its points and shares the outputs
    if (const int rc = grow_owned_slots(out.data(), n_out)) return rc;
    if (robust)
        if (const int rc = t->rcost.grow(t->n_pts, 2 * sizeof(double))) return rc;
    constexpr int G = 4, V = 6;   // the DLT kernel's default geometry (profiles/r09: resources and time)
    const dim3 grid((unsigned)((t->n_pts * G + 255) / 256));
    if (t->cons_ran) {   // the last run had the consensus stage: the same kernels on the table compacted to its inliers
        const int32_t *c_order = tri_launch(t).sorted && t->n_pts < (1ll << 31) ? t->c_order.as<const int32_t>() : nullptr;
        int32_t *info = out[TRI_SLOT_INFO].as<int32_t>();
        HIPCHK(hipEventRecord(t->refine_timer.e0, s));
        if (!robust) {
            hipLaunchKernelGGL((triangulate_refine_kernel<G, V>), grid, dim3(256), 0, s, t->c_cam.as<const int32_t>(), t->c_uv.as<const double2>(),
                               t->c_start.as<const int64_t>(), t->tab.as<const double>(), t->run_pts, t->n_pts, c_order, max_iter, ftol, xtol, gtol,
                               out[TRI_SLOT_POINTS].as<double>(), out[TRI_SLOT_RMS].as<double>(), info, (double *)nullptr);
        } else {
            hipLaunchKernelGGL((triangulate_refine_kernel<G, V, GroupLoss, double *>), grid, dim3(256), 0, s, t->c_cam.as<const int32_t>(),
                               t->c_uv.as<const double2>(), t->c_start.as<const int64_t>(), t->tab.as<const double>(), t->run_pts, t->n_pts, c_order, max_iter,
                               ftol, xtol, gtol, out[TRI_SLOT_POINTS].as<double>(), out[TRI_SLOT_RMS].as<double>(), info, (double *)nullptr,
                               t->refine_loss.args(), t->rcost.as<double>());
        }
        // what callers see: the full view count in info, and the residuals of ALL observations at the returned point, outliers included
        hipLaunchKernelGGL(cons_restore_count_kernel, dim3((unsigned)((t->n_pts + 255) / 256)), dim3(256), 0, s, t->cur_start, t->n_pts, info, 3, 2);
        if (want_resid)
            hipLaunchKernelGGL((tri_score_kernel<TRI_CONS_G, true>), grid, dim3(256), 0, s, t->cur_cam, (const double2 *)t->cur_uv, t->cur_start,
                               t->tab.as<const double>(), t->n_pts, 1, (const double *)out[TRI_SLOT_POINTS].as<double>(), 0.0, (double *)nullptr,
                               out[TRI_SLOT_RESID].as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(t->refine_timer.e1, s));
        t->rlin = {out[TRI_SLOT_RMS].as<double>(), t->c_start.as<const int64_t>(), !robust};   // 0.5 n rms^2 with n the inliers
        t->refine_timer.timed = true;
        t->refine_owned = owned;
        t->refine_valid = true;
        HIPCHK(t->core.fence.after_run(s));
        return PCS_OK;
    }
    // PCS_LOSS_LINEAR launches the kernel a handle without a loss always launched; any other kind its robust twin, which writes the costs itself
    if (!robust) {
        hipExtLaunchKernelGGL((triangulate_refine_kernel<G, V>), grid, dim3(256), 0, s, t->refine_timer.e0, t->refine_timer.e1, 0, t->cur_cam,
                              (const double2 *)t->cur_uv, t->cur_start, t->tab.as<const double>(), t->run_pts, t->n_pts,
                              t->order_valid ? t->order.as<const int32_t>() : nullptr, max_iter, ftol, xtol, gtol, out[TRI_SLOT_POINTS].as<double>(),
                              out[TRI_SLOT_RMS].as<double>(), out[TRI_SLOT_INFO].as<int32_t>(), want_resid ? out[TRI_SLOT_RESID].as<double>() : nullptr);
    } else {
        hipExtLaunchKernelGGL((triangulate_refine_kernel<G, V, GroupLoss, double *>), grid, dim3(256), 0, s, t->refine_timer.e0, t->refine_timer.e1, 0, t->cur_cam,
                              (const double2 *)t->cur_uv, t->cur_start, t->tab.as<const double>(), t->run_pts, t->n_pts,
                              t->order_valid ? t->order.as<const int32_t>() : nullptr, max_iter, ftol, xtol, gtol, out[TRI_SLOT_POINTS].as<double>(),
                              out[TRI_SLOT_RMS].as<double>(), out[TRI_SLOT_INFO].as<int32_t>(), want_resid ? out[TRI_SLOT_RESID].as<double>() : nullptr,
                              t->refine_loss.args(), t->rcost.as<double>());
    }
    HIPCHK(hipGetLastError());
    t->rlin = {out[TRI_SLOT_RMS].as<double>(), t->cur_start, !robust};
    t->refine_timer.timed = true;
    t->refine_owned = owned;
    t->refine_valid = true;
    HIPCHK(t->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_tri_refined(pcs_triangulator *t, double *pts, double *rms, int32_t *info, double *resid) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_refined: NULL handle");
    if (!t->refine_valid) return fail(PCS_ERR_STATE, "pcs_tri_refined: no refinement since the last run (pcs_tri_refine first)");
    const auto out = tri_out_slots(t, pts, rms, info, resid);
    return fetch_slots(t->core, out.data(), TRI_SLOTS, t->refine_owned, t->n_pts != 0, "pcs_tri_refined",
                       "the last refinement wrote some of these outputs to caller buffers (or computed no residuals)");
}

int pcs_tri_set_refine_loss(pcs_triangulator *t, int kind, double f_scale) {
    return set_handle_loss("pcs_tri_set_refine_loss", t ? &t->refine_loss : nullptr, kind, f_scale);
}

int pcs_tri_get_refine_loss(pcs_triangulator *t, int *kind, double *f_scale) {
    return get_handle_loss("pcs_tri_get_refine_loss", t ? &t->refine_loss : nullptr, kind, f_scale);
}

int pcs_tri_refine_costs(pcs_triangulator *t, double *cost) {
    if (!t || !cost) return fail(PCS_ERR_ARG, "pcs_tri_refine_costs: bad arguments");
    if (!t->refine_valid) return fail(PCS_ERR_STATE, "pcs_tri_refine_costs: no refinement since the last run (pcs_tri_refine first)");
    return fetch_costs(t->core, t->rcost, t->rlin, cost, t->n_pts, "pcs_tri_refine_costs");
}

// What the consensus stage of the last run found: blocking, any pointer may be NULL.
int pcs_tri_consensus_results(pcs_triangulator *t, uint8_t *inlier, int32_t *cinfo, double *score) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_consensus_results: NULL handle");
    if (!t->run_valid) return fail(PCS_ERR_STATE, "pcs_tri_consensus_results: no run on the current cameras and observations (pcs_tri_run first)");
    if (!t->cons_ran) return fail(PCS_ERR_STATE, "pcs_tri_consensus_results: the last run had no consensus stage (pcs_tri_set_consensus)");
    const OutSlot out[] = {{1, t->flag, inlier, t->n_obs, sizeof(uint8_t)}, {2, t->cinfo, cinfo, t->n_pts, 4 * sizeof(int32_t)},
                           {4, t->best, score, t->n_pts, sizeof(double)}};
    return fetch_slots(t->core, out, 3, 7, t->n_pts != 0, "pcs_tri_consensus_results", "");
}

int pcs_tri_last_refine_ms(pcs_triangulator *t, float *kernel_ms) {
    return timer_ms("pcs_tri_last_refine_ms", t ? &t->refine_timer : nullptr, kernel_ms, "no refinement has run yet");
}

int pcs_tri_points(pcs_triangulator *t, double *pts) {
    if (!t || !pts) return fail(PCS_ERR_ARG, "pcs_tri_points: bad arguments");
    if (t->n_pts < 0 || (t->n_pts > 0 && (!t->out_owned || !t->pts.p || t->pts.cap < t->n_pts)))
        return fail(PCS_ERR_STATE, "pcs_tri_points: the last run left no handle-owned result (run with d_pts = NULL first)");
    const OutSlot out{1, t->pts, pts, t->n_pts, 3 * sizeof(double)};
    return fetch_slots(t->core, &out, 1, 1, true, "pcs_tri_points", "");
}

int pcs_tri_synchronize(pcs_triangulator *t, void *stream) {
    if (!t) return fail(PCS_ERR_ARG, "pcs_tri_synchronize: bad arguments");
    HIPCHK(hipSetDevice(t->core.device));
    HIPCHK(hipStreamSynchronize(t->core.stream_or(stream)));
    return PCS_OK;
}

int pcs_tri_last_kernel_ms(pcs_triangulator *t, float *kernel_ms) {
    return timer_ms("pcs_tri_last_kernel_ms", t ? &t->timer : nullptr, kernel_ms, "nothing has run yet");
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
