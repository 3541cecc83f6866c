// pcs_stats.inc — host side of the per-group residual statistics (included by pcs_engine.hip; kernels: ba_groupstats.hpp).  Fence, buffers,
// timers and output slots are those of pcs_handle.inc (DESIGN.md, "Batched handles").
extern "C" {
// ---- residual statistics (SURVEY f8): a handle that owns the group index of one detection table (built on the device, kept across
// runs), the gathered errors and the outputs.
struct pcs_residual_stats {
    HandleCore core;
    KernelTimer t_index, t_error, t_stats;
    int64_t count[GS_GROUPINGS] = {0, 0, 0, 0, 1};   // groups per grouping: C, I, K, C I, 1
    int64_t base[GS_GROUPINGS] = {0, 0, 0, 0, 0};    // first flat group of every grouping
    int64_t n_groups = 0;                            // flat groups in all
    int64_t n = -1;                                  // rows of the table; -1: no groups set
    DevBuf perm, start, order, hist, bad;            // the index: (5 n) rows in group order, (n_groups + 1) offsets, visiting order
    DevBuf eg;                                       // the errors in group order (5 n), rewritten by every run
    DevBuf e, ints, vals;                            // handle-owned outputs
    int owned = 0;                                   // PCS_STATS_OUT_* bits: which outputs of the last run are handle-owned
    bool run_valid = false;                          // a run since the groups were last set
};

int pcs_stats_create(pcs_residual_stats **out, int device, int64_t n_cams, int64_t n_imgs, int64_t n_keys) {
    // every flat group and every sort key is an int32
    if (!out || n_cams <= 0 || n_imgs <= 0 || n_keys <= 0 || n_cams > INT32_MAX || n_imgs > INT32_MAX || n_keys > INT32_MAX ||
        n_cams * n_imgs > INT32_MAX || n_cams + n_imgs + n_keys + n_cams * n_imgs + 2 > INT32_MAX)
        return fail(PCS_ERR_ARG, "pcs_stats_create: bad arguments (counts > 0, n_cams + n_imgs + n_keys + n_cams * n_imgs + 2 < 2^31)");
    *out = nullptr;
    if (const int rc = open_device("pcs_stats_create", device)) return rc;
    pcs_residual_stats *p = new pcs_residual_stats();
    p->count[0] = n_cams, p->count[1] = n_imgs, p->count[2] = n_keys, p->count[3] = n_cams * n_imgs;
    for (int g = 1; g < GS_GROUPINGS; ++g) p->base[g] = p->base[g - 1] + p->count[g - 1];
    p->n_groups = p->base[GS_GROUPINGS - 1] + 1;
    hipError_t e = p->core.create(device);
    for (KernelTimer *t : {&p->t_index, &p->t_error, &p->t_stats})
        if (e == hipSuccess) e = t->create();
    if (e == hipSuccess) e = p->start.alloc(p->n_groups + 1, sizeof(int64_t));
    if (e == hipSuccess) e = p->order.alloc(p->n_groups, sizeof(int32_t));
    if (e == hipSuccess) e = p->hist.alloc(GROUP_ORDER_HIST, sizeof(int32_t));
    if (e == hipSuccess) e = p->bad.alloc(1, sizeof(int32_t));
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_stats_create: %s", hipGetErrorString(e));
        pcs_stats_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_stats_destroy(pcs_residual_stats *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->perm, &p->start, &p->order, &p->hist, &p->bad, &p->eg, &p->e, &p->ints, &p->vals}, {&p->t_index, &p->t_error, &p->t_stats});
    delete p;
    return PCS_OK;
}

// buffers that live for one index build
struct StatsScratch {
    DevBuf keys[2], rows[2], blockhist;
    ~StatsScratch() {
        for (DevBuf *b : {&keys[0], &keys[1], &rows[0], &rows[1], &blockhist}) b->release();
    }
};

// The index of a table whose ids are on the device.  Blocking: the ids may be the caller's, and the range check is read back.
static int stats_build_index(pcs_residual_stats *p, const char *who, int64_t n, const int32_t *d_cam, const int32_t *d_img, const int32_t *d_key) {
    const int64_t m = 4 * n, n_chunks = (m + GS_SORT_CHUNK - 1) / GS_SORT_CHUNK, n_sorted = p->n_groups - 1;
    p->n = -1;
    p->run_valid = false;
    StatsScratch sc;
    for (DevBuf *b : {&sc.keys[0], &sc.keys[1], &sc.rows[0], &sc.rows[1]})
        if (const int rc = b->grow(std::max<int64_t>(1, m), sizeof(int32_t))) return rc;
    if (const int rc = sc.blockhist.grow(std::max<int64_t>(1, 256 * n_chunks), sizeof(int32_t))) return rc;
    if (const int rc = p->perm.grow(std::max<int64_t>(1, 5 * n), sizeof(int32_t))) return rc;
    if (const int rc = p->eg.grow(std::max<int64_t>(1, 5 * n), sizeof(double))) return rc;
    hipStream_t s = p->core.stream;
    const int32_t none = INT32_MAX;
    HIPCHK(hipMemcpyAsync(p->bad.p, &none, sizeof none, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(p->t_index.e0, s));   // after every allocation: nothing is queued by a call that fails in one
    int at = 0;   // which of the two (keys, rows) pairs holds the current order
    if (n > 0) {
        hipLaunchKernelGGL(gs_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_cam, d_img, d_key, n, (int32_t)p->count[0], (int32_t)p->count[1],
                           (int32_t)p->count[2], sc.keys[0].as<int32_t>(), sc.rows[0].as<int32_t>(), p->bad.as<int32_t>());
        for (int shift = 0; shift < 32 && (n_sorted - 1) >> shift; shift += 8, at ^= 1) {   // one stable pass per byte of the largest key
            hipLaunchKernelGGL(gs_sort_hist_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, sc.keys[at].as<const int32_t>(), m, shift, sc.blockhist.as<int32_t>(), n_chunks);
            hipLaunchKernelGGL(gs_scan_kernel, dim3(1), dim3(1024), 0, s, sc.blockhist.as<int32_t>(), 256 * n_chunks);
            hipLaunchKernelGGL(gs_sort_scatter_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, sc.keys[at].as<const int32_t>(), sc.rows[at].as<const int32_t>(), m, shift,
                               sc.blockhist.as<const int32_t>(), n_chunks, sc.keys[at ^ 1].as<int32_t>(), sc.rows[at ^ 1].as<int32_t>());
        }
        HIPCHK(hipMemcpyAsync(p->perm.p, sc.rows[at].p, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(gs_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p->perm.as<int32_t>() + m, n);
    }
    hipLaunchKernelGGL(gs_starts_kernel, dim3((unsigned)((m + 1 + 255) / 256)), dim3(256), 0, s, sc.keys[at].as<const int32_t>(), m, n, (int32_t)n_sorted,
                       p->start.as<int64_t>());
    HIPCHK(hipGetLastError());
    if (const int rc = enqueue_group_order(p->start.as<const int64_t>(), p->n_groups, p->hist.as<int32_t>(), p->order.as<int32_t>(), s)) return rc;
    HIPCHK(hipEventRecord(p->t_index.e1, s));
    p->t_index.timed = true;
    int32_t bad = none;
    HIPCHK(hipMemcpyAsync(&bad, p->bad.p, sizeof bad, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad != none) return fail(PCS_ERR_RANGE, "%s: row %d has a camera, image or key outside its count", who, bad);
    p->n = n;
    return PCS_OK;
}

int pcs_stats_set_groups_device(pcs_residual_stats *p, int64_t n, const int32_t *d_cam, const int32_t *d_img, const int32_t *d_key) {
    if (!p || n < 0 || 5 * n > INT32_MAX || (n > 0 && (!d_cam || !d_img || !d_key))) return fail(PCS_ERR_ARG, "pcs_stats_set_groups_device: bad arguments (5 n < 2^31)");
    HIPCHK(p->core.quiesce());
    return stats_build_index(p, "pcs_stats_set_groups_device", n, d_cam, d_img, d_key);
}

int pcs_stats_set_groups(pcs_residual_stats *p, int64_t n, const int32_t *cam, const int32_t *img, const int32_t *key) {
    if (!p || n < 0 || 5 * n > INT32_MAX || (n > 0 && (!cam || !img || !key))) return fail(PCS_ERR_ARG, "pcs_stats_set_groups: bad arguments (5 n < 2^31)");
    const int32_t *ids[3] = {cam, img, key};
    const char *names[3] = {"camera", "image", "key"};
    p->n = -1;   // a refused table leaves no groups behind
    p->run_valid = false;
    for (int g = 0; g < 3; ++g)
        for (int64_t r = 0; r < n; ++r)
            if (ids[g][r] < 0 || ids[g][r] >= p->count[g])
                return fail(PCS_ERR_RANGE, "row %lld has %s %d outside [0,%lld)", (long long)r, names[g], ids[g][r], (long long)p->count[g]);
    HIPCHK(p->core.quiesce());
    StatsScratch sc;   // the ids are needed for the build only
    const HostArray arrays[] = {{sc.keys[0], cam, n, sizeof(int32_t)}, {sc.keys[1], img, n, sizeof(int32_t)}, {sc.rows[0], key, n, sizeof(int32_t)}};
    if (const int rc = upload_host_arrays(p->core, arrays, 3)) return rc;
    return stats_build_index(p, "pcs_stats_set_groups", n, sc.keys[0].as<const int32_t>(), sc.keys[1].as<const int32_t>(), sc.rows[0].as<const int32_t>());
}

static_assert(GS_NO_ORDER_STATISTICS == PCS_STATS_NO_ORDER_STATISTICS && GS_GROUPINGS == PCS_STATS_OVERALL + 1, "flags and groupings of pcs_hip.h");

// the outputs in the order of the PCS_STATS_OUT_* bits
enum { STATS_SLOT_ERRORS, STATS_SLOT_COUNTS, STATS_SLOT_VALUES, STATS_SLOTS };
static std::array<OutSlot, STATS_SLOTS> stats_out_slots(pcs_residual_stats *p, void *o_e, void *o_ints, void *o_vals) {
    return {{{PCS_STATS_OUT_ERRORS, p->e, o_e, p->n, sizeof(double)}, {PCS_STATS_OUT_COUNTS, p->ints, o_ints, p->n_groups, GS_INTS * sizeof(int32_t)},
             {PCS_STATS_OUT_VALUES, p->vals, o_vals, p->n_groups, GS_VALS * sizeof(double)}}};
}

int pcs_stats_run(pcs_residual_stats *p, const double *d_resid, int flags, double *d_errors, int32_t *d_counts, double *d_values, void *stream) {
    if (!p || (flags & ~PCS_STATS_NO_ORDER_STATISTICS)) return fail(PCS_ERR_ARG, "pcs_stats_run: NULL handle or unknown flags");
    if (p->n < 0) return fail(PCS_ERR_STATE, "pcs_stats_run: no groups set (pcs_stats_set_groups first)");
    if (p->n > 0 && !d_resid) return fail(PCS_ERR_ARG, "pcs_stats_run: NULL residuals");
    auto out = stats_out_slots(p, d_errors, d_counts, d_values);
    bool grows = false;
    const int owned = owned_slots(out.data(), STATS_SLOTS, &grows);
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));   // the gathered errors and the outputs are shared between runs
    if (const int rc = grow_owned_slots(out.data(), STATS_SLOTS)) return rc;
    const int64_t n = p->n;
    double *e = out[STATS_SLOT_ERRORS].as<double>();
    HIPCHK(hipEventRecord(p->t_error.e0, s));   // after every allocation: nothing is queued by a call that fails in one
    if (n > 0) hipLaunchKernelGGL(gs_error_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_resid, n, e);
    HIPCHK(hipEventRecord(p->t_error.e1, s));
    HIPCHK(hipEventRecord(p->t_stats.e0, s));
    if (n > 0)
        hipLaunchKernelGGL(gs_gather_kernel, dim3((unsigned)((5 * n + 255) / 256)), dim3(256), 0, s, (const double *)e, p->perm.as<const int32_t>(), 5 * n,
                           p->eg.as<double>());
    hipLaunchKernelGGL(gs_stats_kernel, dim3((unsigned)p->n_groups), dim3(GS_THREADS), 0, s, d_resid, p->eg.as<const double>(), p->perm.as<const int32_t>(),
                       p->start.as<const int64_t>(), p->order.as<const int32_t>(), p->n_groups, flags, out[STATS_SLOT_COUNTS].as<int32_t>(),
                       out[STATS_SLOT_VALUES].as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_stats.e1, s));
    p->t_error.timed = p->t_stats.timed = true;
    p->owned = owned;
    p->run_valid = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_stats_results(pcs_residual_stats *p, int grouping, int32_t *count, int32_t *n_nonfinite, int32_t *argmax, double *sum_e, double *sum_e2, double *sum_ru,
                      double *sum_rv, double *max_e, double *median, double *mad) {
    if (!p || grouping < 0 || grouping >= GS_GROUPINGS) return fail(PCS_ERR_ARG, "pcs_stats_results: NULL handle or unknown grouping (PCS_STATS_BY_* / PCS_STATS_OVERALL)");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_stats_results: no run on the current groups (pcs_stats_run first)");
    // the grouping's stretch of every output row, as slots of its own
    const int64_t G = p->n_groups, b = p->base[grouping], c = p->count[grouping];
    void *host[GS_INTS + GS_VALS] = {count, n_nonfinite, argmax, sum_e, sum_e2, sum_ru, sum_rv, max_e, median, mad};
    DevBuf view[GS_INTS + GS_VALS];
    std::vector<OutSlot> sl;
    for (int j = 0; j < GS_INTS + GS_VALS; ++j) {
        const bool is_int = j < GS_INTS;
        view[j].p = is_int ? (void *)(p->ints.as<int32_t>() + j * G + b) : (void *)(p->vals.as<double>() + (j - GS_INTS) * G + b);
        view[j].cap = c;
        sl.push_back({is_int ? PCS_STATS_OUT_COUNTS : PCS_STATS_OUT_VALUES, view[j], host[j], c, is_int ? sizeof(int32_t) : sizeof(double)});
    }
    return fetch_slots(p->core, sl.data(), (int)sl.size(), p->owned, true, "pcs_stats_results", "the last run wrote these outputs to caller buffers");
}

int pcs_stats_errors(pcs_residual_stats *p, double *errors) {
    if (!p || !errors) return fail(PCS_ERR_ARG, "pcs_stats_errors: bad arguments");
    if (!p->run_valid) return fail(PCS_ERR_STATE, "pcs_stats_errors: no run on the current groups (pcs_stats_run first)");
    const OutSlot sl = {PCS_STATS_OUT_ERRORS, p->e, errors, p->n, sizeof(double)};
    return fetch_slots(p->core, &sl, 1, p->owned, true, "pcs_stats_errors", "the last run wrote the errors to a caller buffer");
}

int pcs_stats_last_kernel_ms(pcs_residual_stats *p, float *index_ms, float *error_ms, float *stats_ms) {
    if (!p) return fail(PCS_ERR_ARG, "pcs_stats_last_kernel_ms: NULL handle");
    if (index_ms)
        if (const int rc = timer_ms("pcs_stats_last_kernel_ms", &p->t_index, index_ms, "no groups have been set yet")) return rc;
    if (error_ms)
        if (const int rc = timer_ms("pcs_stats_last_kernel_ms", &p->t_error, error_ms, "nothing has run yet")) return rc;
    if (stats_ms)
        if (const int rc = timer_ms("pcs_stats_last_kernel_ms", &p->t_stats, stats_ms, "nothing has run yet")) return rc;
    return PCS_OK;
}
}  // extern "C"
