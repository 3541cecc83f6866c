// pcs_rig.inc — host side of the view-graph seeding (included by pcs_engine.hip; kernels: ba_riggraph.hpp).  Fence, buffers, timers and
// output slots are those of pcs_handle.inc (DESIGN.md, "Batched handles").  Every output is handle-owned.
extern "C" {
// ---- view-graph seeding (SURVEY f7): a handle that owns the cameras, the template, the observation copies, the view poses, the
// extrinsics and the outputs of its two runs (edges, scores).
struct pcs_rig_graph {
    HandleCore core;
    KernelTimer t_edges, t_prepare, t_scores;
    int64_t n_cams = 0, n_imgs = 0, n_keys = 0, n_pairs = 0;
    bool have_cams = false, have_template = false, have_poses = false, have_extr = false;
    double centroid[3] = {0, 0, 0}, rho = 0;      // of the template: pbar and the RMS distance from it
    DevBuf intr, pts, pose, mat, ext;             // (C, 9), (K, 3), (C I, 6), (C I, 12), (C, 12)
    DevBuf pair_a, pair_b;                        // the pairs a < b in lexicographic order
    DevBuf key, uv, start, vcam, vim;             // handle-owned copies of the observations (grown on demand)
    DevBuf im_start, im_views;                    // the views of every image, in view order
    int64_t n_obs = 0, n_views = -1;
    bool mat_valid = false;                       // `mat` holds the matrices of `pose`
    DevBuf e_info, e_T, e_stats;                  // outputs of the edge run
    DevBuf W, proj, partial, errors;              // outputs of the score run
    bool edges_valid = false, scores_valid = false;
};

int pcs_rig_create(pcs_rig_graph **out, int device, int64_t n_cams, int64_t n_imgs, int64_t n_keys) {
    if (!out || n_cams <= 0 || n_imgs <= 0 || n_keys <= 0 || n_cams > 46340 || n_imgs > INT32_MAX || n_keys > INT32_MAX || n_cams * n_imgs > INT32_MAX)
        return fail(PCS_ERR_ARG, "pcs_rig_create: bad arguments (n_cams <= 46340: the pairs are counted in 32 bits; n_cams * n_imgs < 2^31)");
    *out = nullptr;
    if (const int rc = open_device("pcs_rig_create", device)) return rc;
    pcs_rig_graph *p = new pcs_rig_graph();
    p->n_cams = n_cams, p->n_imgs = n_imgs, p->n_keys = n_keys;
    p->n_pairs = n_cams * (n_cams - 1) / 2;
    const int64_t ci = n_cams * n_imgs, np = std::max<int64_t>(1, p->n_pairs);
    hipError_t e = p->core.create(device);
    for (KernelTimer *t : {&p->t_edges, &p->t_prepare, &p->t_scores})
        if (e == hipSuccess) e = t->create();
    struct { DevBuf &b; int64_t n; size_t bytes; } fixed[] = {
        {p->intr, n_cams * 9, sizeof(double)},  {p->pts, n_keys * 3, sizeof(double)}, {p->pose, ci * 6, sizeof(double)},  {p->mat, ci * 12, sizeof(double)},
        {p->ext, n_cams * 12, sizeof(double)},  {p->pair_a, np, sizeof(int32_t)},     {p->pair_b, np, sizeof(int32_t)},   {p->e_info, np * 2, sizeof(int32_t)},
        {p->e_T, np * 12, sizeof(double)},      {p->e_stats, np * 3, sizeof(double)}, {p->W, ci * 12, sizeof(double)},    {p->proj, n_cams * 12, sizeof(double)},
        {p->errors, ci, sizeof(double)},        {p->im_start, n_imgs + 1, sizeof(int64_t)}};
    for (auto &f : fixed)
        if (e == hipSuccess) e = f.b.alloc(f.n, f.bytes);
    if (e == hipSuccess && p->n_pairs > 0) {
        std::vector<int32_t> a((size_t)p->n_pairs), b((size_t)p->n_pairs);
        int64_t k = 0;
        for (int64_t i = 0; i < n_cams; ++i)
            for (int64_t j = i + 1; j < n_cams; ++j, ++k) a[k] = (int32_t)i, b[k] = (int32_t)j;
        e = hipMemcpy(p->pair_a.p, a.data(), sizeof(int32_t) * a.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->pair_b.p, b.data(), sizeof(int32_t) * b.size(), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_rig_create: %s", hipGetErrorString(e));
        pcs_rig_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_rig_destroy(pcs_rig_graph *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->intr, &p->pts, &p->pose, &p->mat, &p->ext, &p->pair_a, &p->pair_b, &p->key, &p->uv, &p->start, &p->vcam, &p->vim, &p->im_start,
                     &p->im_views, &p->e_info, &p->e_T, &p->e_stats, &p->W, &p->proj, &p->partial, &p->errors},
                    {&p->t_edges, &p->t_prepare, &p->t_scores});
    delete p;
    return PCS_OK;
}

int pcs_rig_set_cameras(pcs_rig_graph *p, const double *intr) {
    if (!p || !intr) return fail(PCS_ERR_ARG, "pcs_rig_set_cameras: bad arguments");
    if (const int rc = set_fixed_array(p->core, p->intr, intr, sizeof(double) * 9 * p->n_cams)) return rc;
    p->have_cams = true;
    p->scores_valid = false;
    return PCS_OK;
}

int pcs_rig_set_template(pcs_rig_graph *p, const double *points, double *frame) {
    if (!p || !points) return fail(PCS_ERR_ARG, "pcs_rig_set_template: bad arguments");
    double c[3] = {0, 0, 0}, s = 0;
    for (int64_t k = 0; k < p->n_keys; ++k)
        for (int d = 0; d < 3; ++d) c[d] += points[3 * k + d];
    for (int d = 0; d < 3; ++d) c[d] /= (double)p->n_keys;
    for (int64_t k = 0; k < p->n_keys; ++k)
        for (int d = 0; d < 3; ++d) s += (points[3 * k + d] - c[d]) * (points[3 * k + d] - c[d]);
    const double rho = std::sqrt(s / (double)p->n_keys);
    if (!(rho < INFINITY)) return fail(PCS_ERR_ARG, "pcs_rig_set_template: the template points must be finite");
    if (const int rc = set_fixed_array(p->core, p->pts, points, sizeof(double) * 3 * p->n_keys)) return rc;
    for (int d = 0; d < 3; ++d) p->centroid[d] = c[d];
    p->rho = rho;
    if (frame) frame[0] = c[0], frame[1] = c[1], frame[2] = c[2], frame[3] = rho;
    p->have_template = true;
    p->edges_valid = p->scores_valid = false;
    return PCS_OK;
}

int pcs_rig_set_observations(pcs_rig_graph *p, int64_t n_obs, const int32_t *key, const double *uv, int64_t n_views, const int64_t *start_inds,
                             const int32_t *view_cam, const int32_t *view_im) {
    if (!p || n_obs < 0 || n_views < 0 || n_views > INT32_MAX || !start_inds || (n_obs > 0 && (!key || !uv)) || (n_views > 0 && (!view_cam || !view_im)))
        return fail(PCS_ERR_ARG, "pcs_rig_set_observations: bad arguments");
    std::vector<int64_t> im_start((size_t)p->n_imgs + 1, 0);
    const int bad = check_grouped_observations("pcs_rig_set_observations", n_obs, key, p->n_keys, n_views, start_inds, [&](int64_t j) {
        if (const int rc = check_group_entity("view", j, "camera", view_cam[j], p->n_cams)) return rc;
        if (const int rc = check_group_entity("view", j, "image", view_im[j], p->n_imgs)) return rc;
        ++im_start[view_im[j] + 1];
        return (int)PCS_OK;
    });
    if (bad) return bad;
    for (int64_t i = 0; i < p->n_imgs; ++i) im_start[i + 1] += im_start[i];
    std::vector<int32_t> im_views((size_t)n_views);   // a counting sort by image: stable, so an image's views stay in view order
    {
        std::vector<int64_t> next(im_start.begin(), im_start.end() - 1);
        for (int64_t j = 0; j < n_views; ++j) im_views[next[view_im[j]]++] = (int32_t)j;
    }
    HIPCHK(p->core.quiesce());
    p->n_views = -1;
    const HostArray arrays[] = {{p->key, key, n_obs, sizeof(int32_t)},          {p->uv, uv, n_obs, 2 * sizeof(double)},
                                {p->start, start_inds, n_views + 1, sizeof(int64_t)}, {p->vcam, view_cam, n_views, sizeof(int32_t)},
                                {p->vim, view_im, n_views, sizeof(int32_t)},    {p->im_start, im_start.data(), p->n_imgs + 1, sizeof(int64_t)},
                                {p->im_views, im_views.data(), n_views, sizeof(int32_t)}};
    if (const int rc = upload_host_arrays(p->core, arrays, 7)) return rc;
    if (const int rc = p->partial.grow(std::max<int64_t>(1, p->n_cams * n_views), sizeof(double))) return rc;
    p->n_obs = n_obs;
    p->n_views = n_views;
    p->scores_valid = false;
    return PCS_OK;
}

int pcs_rig_set_view_poses(pcs_rig_graph *p, const double *poses) {
    if (!p || !poses) return fail(PCS_ERR_ARG, "pcs_rig_set_view_poses: bad arguments");
    if (const int rc = set_fixed_array(p->core, p->pose, poses, sizeof(double) * 6 * p->n_cams * p->n_imgs)) return rc;
    p->have_poses = true;
    p->mat_valid = p->edges_valid = p->scores_valid = false;
    return PCS_OK;
}

int pcs_rig_set_extrinsics(pcs_rig_graph *p, const double *ext) {
    if (!p || !ext) return fail(PCS_ERR_ARG, "pcs_rig_set_extrinsics: bad arguments");
    if (const int rc = set_fixed_array(p->core, p->ext, ext, sizeof(double) * 12 * p->n_cams)) return rc;
    p->have_extr = true;
    p->scores_valid = false;
    return PCS_OK;
}

// lanes per (view, candidate) group of the scoring kernel (profiles/r13: kernel resources)
constexpr int RIG_G = 16;

static void rig_enqueue_matrices(pcs_rig_graph *p, hipStream_t s) {
    if (p->mat_valid) return;
    const int64_t ci = p->n_cams * p->n_imgs;
    hipLaunchKernelGGL(rig_view_matrix_kernel, dim3((unsigned)((ci + 255) / 256)), dim3(256), 0, s, p->pose.as<const double>(), ci, p->mat.as<double>());
    p->mat_valid = true;
}

int pcs_rig_run_edges(pcs_rig_graph *p, void *stream) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_rig_run_edges: NULL handle");
    if (!p->have_template || !p->have_poses) return fail(PCS_ERR_STATE, "pcs_rig_run_edges: template or view poses not set");
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, false));
    HIPCHK(hipEventRecord(p->t_edges.e0, s));
    rig_enqueue_matrices(p, s);
    if (p->n_pairs > 0)
        hipLaunchKernelGGL((rig_edge_kernel<RIG_TILE>), dim3((unsigned)p->n_pairs), dim3(RIG_THREADS), 0, s, p->mat.as<const double>(), p->pair_a.as<const int32_t>(),
                           p->pair_b.as<const int32_t>(), p->n_imgs, p->centroid[0], p->centroid[1], p->centroid[2], p->rho * p->rho / 3.0,
                           p->e_info.as<int32_t>(), p->e_T.as<double>(), p->e_stats.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_edges.e1, s));
    p->t_edges.timed = true;
    p->edges_valid = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

enum { RIG_OUT_EDGE_INFO = 1, RIG_OUT_EDGE_T = 2, RIG_OUT_EDGE_STATS = 4, RIG_OUT_W = 8, RIG_OUT_ERRORS = 16, RIG_OUT_PARTIAL = 32 };

int pcs_rig_edges(pcs_rig_graph *p, int32_t *info, double *T, double *stats) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_rig_edges: NULL handle");
    if (!p->edges_valid) return fail(PCS_ERR_STATE, "pcs_rig_edges: no edge run on the current template and view poses (pcs_rig_run_edges first)");
    const OutSlot out[] = {{RIG_OUT_EDGE_INFO, p->e_info, info, p->n_pairs, 2 * sizeof(int32_t)}, {RIG_OUT_EDGE_T, p->e_T, T, p->n_pairs, 12 * sizeof(double)},
                           {RIG_OUT_EDGE_STATS, p->e_stats, stats, p->n_pairs, 3 * sizeof(double)}};
    return fetch_slots(p->core, out, 3, ~0, p->n_pairs != 0, "pcs_rig_edges", "");
}

int pcs_rig_run_scores(pcs_rig_graph *p, void *stream) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_rig_run_scores: NULL handle");
    if (!p->have_cams || !p->have_template || !p->have_poses || !p->have_extr || p->n_views < 0)
        return fail(PCS_ERR_STATE, "pcs_rig_run_scores: cameras, template, observations, view poses or extrinsics not set");
    const int64_t ci = p->n_cams * p->n_imgs, nv = p->n_views;
    if ((nv * p->n_cams * RIG_G + 255) / 256 > INT32_MAX) return fail(PCS_ERR_ARG, "pcs_rig_run_scores: views x cameras exceeds one launch");
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, false));
    HIPCHK(hipEventRecord(p->t_prepare.e0, s));
    rig_enqueue_matrices(p, s);
    hipLaunchKernelGGL(rig_prepare_kernel, dim3((unsigned)((ci + 255) / 256)), dim3(256), 0, s, p->ext.as<const double>(), p->intr.as<const double>(),
                       p->mat.as<const double>(), p->n_cams, p->n_imgs, p->W.as<double>(), p->proj.as<double>());
    HIPCHK(hipEventRecord(p->t_prepare.e1, s));
    HIPCHK(hipEventRecord(p->t_scores.e0, s));
    if (nv > 0) {
        const int64_t groups = nv * p->n_cams;
        hipLaunchKernelGGL((rig_score_kernel<RIG_G>), dim3((unsigned)((groups * RIG_G + 255) / 256)), dim3(256), 0, s, p->key.as<const int32_t>(),
                           p->uv.as<const double2>(), p->start.as<const int64_t>(), p->vcam.as<const int32_t>(), p->vim.as<const int32_t>(),
                           p->W.as<const double>(), p->proj.as<const double>(), p->intr.as<const double>(), p->pts.as<const double>(), nv, p->n_cams,
                           p->n_imgs, p->partial.as<double>());
    }
    hipLaunchKernelGGL(rig_image_sum_kernel, dim3((unsigned)((ci + 255) / 256)), dim3(256), 0, s, p->partial.as<const double>(), p->im_start.as<const int64_t>(),
                       p->im_views.as<const int32_t>(), p->W.as<const double>(), p->n_cams, p->n_imgs, nv, p->errors.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_scores.e1, s));
    p->t_prepare.timed = p->t_scores.timed = true;
    p->scores_valid = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_rig_results(pcs_rig_graph *p, double *W, double *errors, double *partial) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_rig_results: NULL handle");
    if (!p->scores_valid) return fail(PCS_ERR_STATE, "pcs_rig_results: no score run on the current inputs (pcs_rig_run_scores first)");
    const int64_t ci = p->n_cams * p->n_imgs;
    const OutSlot out[] = {{RIG_OUT_W, p->W, W, ci, 12 * sizeof(double)}, {RIG_OUT_ERRORS, p->errors, errors, ci, sizeof(double)},
                           {RIG_OUT_PARTIAL, p->partial, partial, p->n_cams * p->n_views, sizeof(double)}};
    return fetch_slots(p->core, out, 3, ~0, true, "pcs_rig_results", "");
}

int pcs_rig_last_kernel_ms(pcs_rig_graph *p, float *edges_ms, float *prepare_ms, float *scores_ms) {
    if (!p || (!edges_ms && !prepare_ms && !scores_ms)) return fail(PCS_ERR_ARG, "pcs_rig_last_kernel_ms: bad arguments");
    if (edges_ms)
        if (const int rc = timer_ms("pcs_rig_last_kernel_ms", &p->t_edges, edges_ms, "no edge run yet")) return rc;
    if (prepare_ms)
        if (const int rc = timer_ms("pcs_rig_last_kernel_ms", &p->t_prepare, prepare_ms, "no score run yet")) return rc;
    if (scores_ms)
        if (const int rc = timer_ms("pcs_rig_last_kernel_ms", &p->t_scores, scores_ms, "no score run yet")) return rc;
    return PCS_OK;
}
}  // extern "C"
