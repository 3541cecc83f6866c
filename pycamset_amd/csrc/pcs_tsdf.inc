// pcs_tsdf.inc — host side of the TSDF volume and the surface-nets extraction (included by pcs_engine.hip behind pcs_fusion.inc; kernels:
// ba_tsdf.hpp).  The handle owns the view table (the rows of pcs_fuse_set_views), the volume (sum and weight per node), the view list
// of the last integration and the extraction's workspace: the cell flags, the cell -> vertex map, the quad flags and the block counts
// and offsets of the two compactions (stereo_count_kernel / stereo_scan_kernel, unchanged).  Depth maps, vertices and quads are the
// caller's device buffers.  The ray-cast (kernels: ba_tsdf_raycast.hpp) adds the table of the render views and the brick mask; it reads
// the volume only.  The colour stage (kernels: ba_tsdf_colour.hpp) adds the table of the source views and of its own render views; it
// reads the volume for the point normals only.  Fence and timers are those of pcs_handle.inc (DESIGN.md, "Batched handles").
struct pcs_tsdf_volume {
    HandleCore core;
    KernelTimer t_integrate, t_count, t_write, t_mask, t_cast, t_pnormal, t_colour;
    DevBuf views, list, sum, weight, cflag, map, qflag, blk, coff, qoff, rviews, brick, cviews, crviews;
    int64_t n_views = 0, n_integrated = 0;   // n_integrated: views integrated since the volume was zeroed (no weight can exceed it)
    int width = 0, height = 0;
    TsdfGrid g{};
    bool have_grid = false, f32 = true, counted = false;   // counted: an extract_count on the volume as it stands
    int min_weight = 0;
    int64_t n_vertices = 0, n_quads = 0;
    TsdfRaycastArgs last_cast{};   // the last cast, for pcs_tsdf_raycast_count_samples; cast_views = 0: none on the volume as it stands
    int64_t cast_views = 0;
    int64_t nodes() const { return (int64_t)g.nx * g.ny * g.nz; }
    int64_t cells() const { return (int64_t)(g.nx - 1) * (g.ny - 1) * (g.nz - 1); }
};

static_assert(TSDF_MAX_DIM == PCS_TSDF_MAX_DIM && TSDF_MAX_WEIGHT == PCS_TSDF_MAX_WEIGHT, "limits of pcs_hip.h");
// the compaction's limits admit the largest grid: 3 nz "views" in blockIdx.y, and the one-workgroup scan walks any number of blocks
static_assert(3 * TSDF_MAX_DIM <= 65535 && 3 * TSDF_MAX_DIM <= STEREO_MAX_PAIRS, "quad flags as 3 nz views of the compaction");

// Every argument of pcs_tsdf_set_grid but the handle: nothing here touches the device.
static int tsdf_check_grid(const char *who, const double *origin, double voxel, int nx, int ny, int nz, int sum_dtype) {
    if (!origin) return fail(PCS_ERR_ARG, "%s: origin (3) must be given", who);
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(origin[c])) return fail(PCS_ERR_ARG, "%s: origin is not finite", who);
    if (!std::isfinite(voxel) || !(voxel > 0.0)) return fail(PCS_ERR_ARG, "%s: voxel must be finite and > 0 (got %g)", who, voxel);
    const int d[3] = {nx, ny, nz};
    for (int c = 0; c < 3; ++c)
        if (d[c] < 1 || d[c] > TSDF_MAX_DIM) return fail(PCS_ERR_ARG, "%s: n%c %d outside [1, %d]", who, "xyz"[c], d[c], TSDF_MAX_DIM);
    if (sum_dtype != PCS_F64 && sum_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: sum_dtype PCS_F64 or PCS_F32", who);
    return PCS_OK;
}

// Every argument of pcs_tsdf_integrate that needs no handle.
static int tsdf_check_integrate(const char *who, const void *d_depth, int depth_dtype, const int32_t *views, int64_t n_list, double trunc) {
    if (depth_dtype != PCS_F64 && depth_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: depth_dtype PCS_F64 or PCS_F32", who);
    if (!std::isfinite(trunc) || !(trunc > 0.0)) return fail(PCS_ERR_ARG, "%s: trunc must be finite and > 0 (got %g)", who, trunc);
    if (views && (n_list < 0 || n_list > TSDF_MAX_WEIGHT)) return fail(PCS_ERR_ARG, "%s: n_list %lld outside [0, %d]", who, (long long)n_list, TSDF_MAX_WEIGHT);
    if (!d_depth) return fail(PCS_ERR_ARG, "%s: d_depth must be given", who);
    return PCS_OK;
}

// Every argument of pcs_tsdf_raycast that needs no handle (the grid is looked at with the handle: step is held against its voxel).
static int tsdf_check_raycast(const char *who, int64_t n_views, int width, int height, const double *K, const double *P, int min_weight, double step, double z_near,
                              double z_far, const void *d_depth, int depth_dtype, int flags) {
    if (const int rc = fuse_check_views(who, n_views, width, height, K, P)) return rc;
    if (min_weight < 1 || min_weight > TSDF_MAX_WEIGHT) return fail(PCS_ERR_ARG, "%s: min_weight %d outside [1, %d]", who, min_weight, TSDF_MAX_WEIGHT);
    if (!std::isfinite(step) || !(step > 0.0)) return fail(PCS_ERR_ARG, "%s: step must be finite and > 0 (got %g)", who, step);
    if (!(z_near >= 0.0) || !(z_near < z_far)) return fail(PCS_ERR_ARG, "%s: z_near and z_far must satisfy 0 <= z_near < z_far (got %g, %g)", who, z_near, z_far);
    if (depth_dtype != PCS_F64 && depth_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: depth_dtype PCS_F64 or PCS_F32", who);
    if (!d_depth) return fail(PCS_ERR_ARG, "%s: d_depth must be given", who);
    if (flags & ~PCS_TSDF_RAYCAST_NO_SKIP) return fail(PCS_ERR_ARG, "%s: flags %d has bits other than PCS_TSDF_RAYCAST_NO_SKIP", who, flags);
    return PCS_OK;
}

// The table of the render views: per view K = [fx, cx, fy, cy], the nine entries of R row-major, then the centre
// C_a = -((R_0a t_0 + R_1a t_1) + R_2a t_2), in plain double operations in that order
static std::vector<double> tsdf_render_rows(int64_t n_views, const double *K, const double *P) {
    std::vector<double> rows(16 * (size_t)n_views);
    for (int64_t v = 0; v < n_views; ++v) {
        double *o = rows.data() + 16 * v;
        const double *Pv = P + 12 * v;
        std::copy(K + 4 * v, K + 4 * v + 4, o);
        for (int k = 0; k < 9; ++k) o[4 + k] = Pv[k + k / 3];
        for (int a = 0; a < 3; ++a) {
            volatile double m0 = Pv[a] * Pv[3], m1 = Pv[4 + a] * Pv[7], m2 = Pv[8 + a] * Pv[11];   // each product rounded on its own: no contraction on the host either
            volatile double sum = m0 + m1;
            sum = sum + m2;
            o[13 + a] = -sum;
        }
    }
    return rows;
}

static TsdfExtractArgs tsdf_extract_args(const pcs_tsdf_volume *p) {
    TsdfExtractArgs a{};
    a.sum = p->sum.p, a.weight = p->weight.as<const uint16_t>(), a.g = p->g, a.min_weight = p->min_weight, a.map = p->map.as<int32_t>();
    return a;
}

extern "C" {
int pcs_tsdf_create(pcs_tsdf_volume **out, int device) {
    if (!out) return fail(PCS_ERR_ARG, "pcs_tsdf_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_tsdf_create", device)) return rc;
    pcs_tsdf_volume *p = new pcs_tsdf_volume();
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->t_integrate.create();
    if (e == hipSuccess) e = p->t_count.create();
    if (e == hipSuccess) e = p->t_write.create();
    if (e == hipSuccess) e = p->t_mask.create();
    if (e == hipSuccess) e = p->t_cast.create();
    if (e == hipSuccess) e = p->t_pnormal.create();
    if (e == hipSuccess) e = p->t_colour.create();
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_tsdf_create: %s", hipGetErrorString(e));
        pcs_tsdf_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_tsdf_destroy(pcs_tsdf_volume *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->views, &p->list, &p->sum, &p->weight, &p->cflag, &p->map, &p->qflag, &p->blk, &p->coff, &p->qoff, &p->rviews, &p->brick,
                     &p->cviews, &p->crviews},
                    {&p->t_integrate, &p->t_count, &p->t_write, &p->t_mask, &p->t_cast, &p->t_pnormal, &p->t_colour});
    delete p;
    return PCS_OK;
}

// K and P are HOST arrays and are copied: the arguments and checks of pcs_fuse_set_views.  The volume is kept.
int pcs_tsdf_set_views(pcs_tsdf_volume *p, int64_t n_views, int width, int height, const double *K, const double *P) {
    const char *who = "pcs_tsdf_set_views";
    if (const int rc = fuse_check_views(who, n_views, width, height, K, P)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    const std::vector<double> rows = fuse_view_rows(n_views, K, P);
    HIPCHK(p->core.quiesce());   // a queued integration may still read the old table
    p->n_views = 0;
    const HostArray up[] = {{p->views, rows.data(), 16 * n_views, sizeof(double)}};
    if (const int rc = upload_host_arrays(p->core, up, 1)) return rc;
    p->n_views = n_views, p->width = width, p->height = height;
    return PCS_OK;
}

static int tsdf_zero(pcs_tsdf_volume *p) {
    const int64_t N = p->nodes();
    HIPCHK(hipMemsetAsync(p->sum.p, 0, (size_t)N * (p->f32 ? sizeof(float) : sizeof(double)), p->core.stream));
    HIPCHK(hipMemsetAsync(p->weight.p, 0, (size_t)N * sizeof(uint16_t), p->core.stream));
    HIPCHK(hipStreamSynchronize(p->core.stream));
    p->n_integrated = 0, p->counted = false, p->cast_views = 0;
    return PCS_OK;
}

// Allocates the volume and zeroes it.
int pcs_tsdf_set_grid(pcs_tsdf_volume *p, const double *origin, double voxel, int nx, int ny, int nz, int sum_dtype) {
    const char *who = "pcs_tsdf_set_grid";
    if (const int rc = tsdf_check_grid(who, origin, voxel, nx, ny, nz, sum_dtype)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    HIPCHK(p->core.quiesce());
    p->have_grid = p->counted = false;
    p->cast_views = 0;
    const int64_t N = (int64_t)nx * ny * nz;
    if (const int rc = p->sum.grow(N * (sum_dtype == PCS_F32 ? 1 : 2), sizeof(float))) return rc;   // capacity counted in 4-byte words: either dtype fits
    if (const int rc = p->weight.grow(N, sizeof(uint16_t))) return rc;
    p->g.o[0] = origin[0], p->g.o[1] = origin[1], p->g.o[2] = origin[2], p->g.s = voxel, p->g.nx = nx, p->g.ny = ny, p->g.nz = nz;
    p->f32 = sum_dtype == PCS_F32;
    if (const int rc = tsdf_zero(p)) return rc;
    p->have_grid = true;
    return PCS_OK;
}

int pcs_tsdf_reset(pcs_tsdf_volume *p) {
    const char *who = "pcs_tsdf_reset";
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (!p->have_grid) return fail(PCS_ERR_STATE, "%s: pcs_tsdf_set_grid comes first", who);
    HIPCHK(p->core.quiesce());
    return tsdf_zero(p);
}

// `views` is a HOST list of indices into the view table (NULL: all views in order); it is copied.
int pcs_tsdf_integrate(pcs_tsdf_volume *p, const void *d_depth, int depth_dtype, const int32_t *views, int64_t n_list, double trunc, void *stream) {
    const char *who = "pcs_tsdf_integrate";
    if (const int rc = tsdf_check_integrate(who, d_depth, depth_dtype, views, n_list, trunc)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (p->n_views == 0 || !p->have_grid) return fail(PCS_ERR_STATE, "%s: pcs_tsdf_set_views and pcs_tsdf_set_grid come first", who);
    const int64_t m = views ? n_list : p->n_views;
    for (int64_t l = 0; views && l < m; ++l)
        if (views[l] < 0 || views[l] >= p->n_views) return fail(PCS_ERR_ARG, "%s: views entry %lld is %d, outside [0, %lld)", who, (long long)l, views[l], (long long)p->n_views);
    if (p->n_integrated + m > TSDF_MAX_WEIGHT)
        return fail(PCS_ERR_ARG, "%s: views: %lld more after %lld integrated could take a weight past %d", who, (long long)m, (long long)p->n_integrated, TSDF_MAX_WEIGHT);
    if (m == 0) return PCS_OK;   // an empty list: the volume stays as it is
    HIPCHK(hipSetDevice(p->core.device));
    if (views) HIPCHK(p->core.quiesce());   // a queued integration may still read the old list
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, views && p->list.grows(m)));
    if (views) {
        if (const int rc = p->list.grow(m, sizeof(int32_t))) return rc;
        HIPCHK(hipMemcpy(p->list.p, views, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice));
    }
    TsdfIntegrateArgs a{};
    a.views = p->views.as<const double>(), a.list = views ? p->list.as<const int32_t>() : nullptr, a.n_list = (int)m, a.depth = d_depth, a.W = p->width, a.H = p->height;
    a.g = p->g, a.trunc = trunc, a.sum = p->sum.p, a.weight = p->weight.as<uint16_t>();
    const dim3 grid((unsigned)((p->g.nx + TSDF_TX - 1) / TSDF_TX), (unsigned)((p->g.ny + TSDF_TY - 1) / TSDF_TY), (unsigned)p->g.nz), block(TSDF_TX, TSDF_TY);
    p->counted = false, p->cast_views = 0;
    p->n_integrated += m;
    HIPCHK(hipEventRecord(p->t_integrate.e0, s));
    if (depth_dtype == PCS_F32) {
        if (p->f32) hipLaunchKernelGGL((tsdf_integrate_kernel<float, float>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((tsdf_integrate_kernel<float, double>), grid, block, 0, s, a);
    } else {
        if (p->f32) hipLaunchKernelGGL((tsdf_integrate_kernel<double, float>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((tsdf_integrate_kernel<double, double>), grid, block, 0, s, a);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_integrate.e1, s));
    p->t_integrate.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

int pcs_tsdf_volume_ptrs(pcs_tsdf_volume *p, void **d_sum, uint16_t **d_weight) {
    const char *who = "pcs_tsdf_volume_ptrs";
    if (!p || (!d_sum && !d_weight)) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (!p->have_grid) return fail(PCS_ERR_STATE, "%s: pcs_tsdf_set_grid comes first", who);
    if (d_sum) *d_sum = p->sum.p;
    if (d_weight) *d_weight = p->weight.as<uint16_t>();
    return PCS_OK;
}

// Classification, numbering and the quad flags, with the two scans; the two totals come back to the host (blocking).
int pcs_tsdf_extract_count(pcs_tsdf_volume *p, int min_weight, int64_t *n_vertices, int64_t *n_quads, void *stream) {
    const char *who = "pcs_tsdf_extract_count";
    if (min_weight < 1 || min_weight > TSDF_MAX_WEIGHT) return fail(PCS_ERR_ARG, "%s: min_weight %d outside [1, %d]", who, min_weight, TSDF_MAX_WEIGHT);
    if (!n_vertices || !n_quads) return fail(PCS_ERR_ARG, "%s: n_vertices and n_quads must be given", who);
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (!p->have_grid) return fail(PCS_ERR_STATE, "%s: pcs_tsdf_set_grid comes first", who);
    p->counted = false;
    p->min_weight = min_weight, p->n_vertices = p->n_quads = 0;
    const int64_t C = p->cells(), N = p->nodes();
    if (C > 0) {
        const int cz = p->g.nz - 1, qz = 3 * p->g.nz;
        const int64_t cHW = (int64_t)(p->g.nx - 1) * (p->g.ny - 1), qHW = (int64_t)p->g.nx * p->g.ny;
        const int64_t cblk = (cHW + STEREO_PIX_PER_BLOCK - 1) / STEREO_PIX_PER_BLOCK, qblk = (qHW + STEREO_PIX_PER_BLOCK - 1) / STEREO_PIX_PER_BLOCK;
        const int64_t cNB = cblk * cz, qNB = qblk * qz;
        const bool grows = p->cflag.grows(C) || p->map.grows(C) || p->qflag.grows(3 * N) || p->blk.grows(std::max(cNB, qNB)) || p->coff.grows(cNB + 1) || p->qoff.grows(qNB + 1);
        HIPCHK(hipSetDevice(p->core.device));
        hipStream_t s = p->core.stream_or(stream);
        HIPCHK(p->core.fence.before_run(s, grows));
        if (const int rc = p->cflag.grow(C, 1)) return rc;
        if (const int rc = p->map.grow(C, sizeof(int32_t))) return rc;
        if (const int rc = p->qflag.grow(3 * N, 1)) return rc;
        if (const int rc = p->blk.grow(std::max(cNB, qNB), sizeof(int32_t))) return rc;
        if (const int rc = p->coff.grow(cNB + 1, sizeof(int64_t))) return rc;
        if (const int rc = p->qoff.grow(qNB + 1, sizeof(int64_t))) return rc;
        TsdfExtractArgs a = tsdf_extract_args(p);
        const dim3 cgrid((unsigned)cblk, (unsigned)cz), qgrid((unsigned)qblk, (unsigned)qz), block(STEREO_PIX_PER_BLOCK);
        HIPCHK(hipEventRecord(p->t_count.e0, s));
        a.flag = p->cflag.as<uint8_t>(), a.nblk = (int)cblk, a.off = p->coff.as<const int64_t>();
        if (p->f32) hipLaunchKernelGGL(tsdf_classify_kernel<float>, cgrid, block, 0, s, a);
        else hipLaunchKernelGGL(tsdf_classify_kernel<double>, cgrid, block, 0, s, a);
        hipLaunchKernelGGL(stereo_count_kernel, cgrid, block, 0, s, p->cflag.as<const uint8_t>(), cHW, (int)cblk, p->blk.as<int32_t>());
        hipLaunchKernelGGL(stereo_scan_kernel, dim3(1), dim3(1024), 0, s, p->blk.as<const int32_t>(), cNB, (int)cblk, cz, p->coff.as<int64_t>(), (int64_t *)nullptr);
        hipLaunchKernelGGL(tsdf_number_kernel, cgrid, block, 0, s, a);
        a.flag = p->qflag.as<uint8_t>(), a.nblk = (int)qblk, a.off = p->qoff.as<const int64_t>();
        if (p->f32) hipLaunchKernelGGL(tsdf_quad_flag_kernel<float>, qgrid, block, 0, s, a);
        else hipLaunchKernelGGL(tsdf_quad_flag_kernel<double>, qgrid, block, 0, s, a);
        hipLaunchKernelGGL(stereo_count_kernel, qgrid, block, 0, s, p->qflag.as<const uint8_t>(), qHW, (int)qblk, p->blk.as<int32_t>());
        hipLaunchKernelGGL(stereo_scan_kernel, dim3(1), dim3(1024), 0, s, p->blk.as<const int32_t>(), qNB, (int)qblk, qz, p->qoff.as<int64_t>(), (int64_t *)nullptr);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(p->t_count.e1, s));
        p->t_count.timed = true;
        HIPCHK(hipMemcpyAsync(&p->n_vertices, p->coff.as<const int64_t>() + cNB, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&p->n_quads, p->qoff.as<const int64_t>() + qNB, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIPCHK(p->core.fence.after_run(s));
        HIPCHK(hipStreamSynchronize(s));
    }
    *n_vertices = p->n_vertices, *n_quads = p->n_quads;
    p->counted = true;
    return PCS_OK;
}

// Fills d_vertices (n_vertices, 3) of vertex_dtype and d_quads (n_quads, 4) int32: the sizes the count returned.
int pcs_tsdf_extract_write(pcs_tsdf_volume *p, void *d_vertices, int vertex_dtype, int32_t *d_quads, void *stream) {
    const char *who = "pcs_tsdf_extract_write";
    if (vertex_dtype != PCS_F64 && vertex_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: vertex_dtype PCS_F64 or PCS_F32", who);
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (!p->have_grid || !p->counted) return fail(PCS_ERR_ARG, "%s: no pcs_tsdf_extract_count on the volume as it stands", who);
    if ((p->n_vertices > 0 && !d_vertices) || (p->n_quads > 0 && !d_quads)) return fail(PCS_ERR_ARG, "%s: d_vertices and d_quads must be given", who);
    if (p->n_vertices == 0) return PCS_OK;   // no vertex, so no quad
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, false));
    const int cz = p->g.nz - 1, qz = 3 * p->g.nz;
    const int64_t cHW = (int64_t)(p->g.nx - 1) * (p->g.ny - 1), qHW = (int64_t)p->g.nx * p->g.ny;
    const int64_t cblk = (cHW + STEREO_PIX_PER_BLOCK - 1) / STEREO_PIX_PER_BLOCK, qblk = (qHW + STEREO_PIX_PER_BLOCK - 1) / STEREO_PIX_PER_BLOCK;
    const dim3 cgrid((unsigned)cblk, (unsigned)cz), qgrid((unsigned)qblk, (unsigned)qz), block(STEREO_PIX_PER_BLOCK);
    TsdfExtractArgs a = tsdf_extract_args(p);
    a.vertices = d_vertices, a.quads = d_quads;
    HIPCHK(hipEventRecord(p->t_write.e0, s));
    const bool v32 = vertex_dtype == PCS_F32;
    if (v32 && p->f32) hipLaunchKernelGGL((tsdf_vertex_kernel<float, float>), cgrid, block, 0, s, a);
    else if (v32) hipLaunchKernelGGL((tsdf_vertex_kernel<float, double>), cgrid, block, 0, s, a);
    else if (p->f32) hipLaunchKernelGGL((tsdf_vertex_kernel<double, float>), cgrid, block, 0, s, a);
    else hipLaunchKernelGGL((tsdf_vertex_kernel<double, double>), cgrid, block, 0, s, a);
    if (p->n_quads > 0) {
        a.flag = p->qflag.as<uint8_t>(), a.nblk = (int)qblk, a.off = p->qoff.as<const int64_t>();
        if (p->f32) hipLaunchKernelGGL(tsdf_quad_write_kernel<float>, qgrid, block, 0, s, a);
        else hipLaunchKernelGGL(tsdf_quad_write_kernel<double>, qgrid, block, 0, s, a);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_write.e1, s));
    p->t_write.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

// Depth, normal and status maps of n_views render views by marching the volume (the rule: include/pcs_hip.h).  K and P are HOST arrays
// and are copied.  The volume, the integration's view table and a preceding count are left as they are.
int pcs_tsdf_raycast(pcs_tsdf_volume *p, int64_t n_views, int width, int height, const double *K, const double *P, int min_weight, double step, double z_near,
                     double z_far, void *d_depth, int depth_dtype, float *d_normal, uint8_t *d_status, int flags, void *stream) {
    const char *who = "pcs_tsdf_raycast";
    if (const int rc = tsdf_check_raycast(who, n_views, width, height, K, P, min_weight, step, z_near, z_far, d_depth, depth_dtype, flags)) return rc;
    if (n_views > 65535) return fail(PCS_ERR_ARG, "%s: n_views %lld above 65535", who, (long long)n_views);   // blockIdx.z; fuse_check_views stops at 32767 already
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (!p->have_grid) return fail(PCS_ERR_ARG, "%s: no grid: pcs_tsdf_set_grid comes first", who);
    if (!(step >= p->g.s / 64.0)) return fail(PCS_ERR_ARG, "%s: step %g is below voxel / 64 = %g", who, step, p->g.s / 64.0);
    const std::vector<double> rows = tsdf_render_rows(n_views, K, P);
    const bool cells = p->g.nx >= 2 && p->g.ny >= 2 && p->g.nz >= 2;   // no cells: every ray misses and no mask is made
    const bool skip = cells && !(flags & PCS_TSDF_RAYCAST_NO_SKIP);
    const int bx = cells ? (p->g.nx - 1 + 7) >> 3 : 1, by = cells ? (p->g.ny - 1 + 7) >> 3 : 1, bz = cells ? (p->g.nz - 1 + 7) >> 3 : 1;
    const int64_t n_bricks = (int64_t)bx * by * bz;
    HIPCHK(p->core.quiesce());   // a queued cast may still read the old table
    p->cast_views = 0;
    const HostArray up[] = {{p->rviews, rows.data(), 16 * n_views, sizeof(double)}};
    if (const int rc = upload_host_arrays(p->core, up, 1)) return rc;
    if (skip)
        if (const int rc = p->brick.grow(n_bricks, 1)) return rc;
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, false));
    if (skip) {
        TsdfMaskArgs m{};
        m.sum = p->sum.p, m.weight = p->weight.as<const uint16_t>(), m.g = p->g, m.bx = bx, m.by = by, m.bz = bz, m.min_weight = min_weight, m.mask = p->brick.as<uint8_t>();
        const dim3 grid((unsigned)((p->g.nx + TSDF_TX - 1) / TSDF_TX), (unsigned)((p->g.ny + TSDF_TY - 1) / TSDF_TY), (unsigned)p->g.nz), block(TSDF_TX, TSDF_TY);
        HIPCHK(hipEventRecord(p->t_mask.e0, s));
        HIPCHK(hipMemsetAsync(p->brick.p, 0, (size_t)n_bricks, s));
        if (p->f32) hipLaunchKernelGGL(tsdf_brick_mask_kernel<float>, grid, block, 0, s, m);
        else hipLaunchKernelGGL(tsdf_brick_mask_kernel<double>, grid, block, 0, s, m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(p->t_mask.e1, s));
    }
    p->t_mask.timed = skip;
    TsdfRaycastArgs a{};
    a.views = p->rviews.as<const double>(), a.sum = p->sum.p, a.weight = p->weight.as<const uint16_t>(), a.mask = skip ? p->brick.as<const uint8_t>() : nullptr;
    a.g = p->g, a.bx = bx, a.by = by, a.W = width, a.H = height, a.min_weight = min_weight, a.step = step, a.z_near = z_near, a.z_far = z_far;
    a.depth = d_depth, a.normal = d_normal, a.status = d_status;
    const dim3 grid((unsigned)((width + TSDF_RAY_BLOCK - 1) / TSDF_RAY_BLOCK), (unsigned)((height + TSDF_RAY_BLOCK - 1) / TSDF_RAY_BLOCK), (unsigned)n_views),
        block(TSDF_RAY_BLOCK * TSDF_RAY_BLOCK);
    HIPCHK(hipEventRecord(p->t_cast.e0, s));
    if (depth_dtype == PCS_F32) {
        if (p->f32) hipLaunchKernelGGL((tsdf_raycast_kernel<float, float>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((tsdf_raycast_kernel<double, float>), grid, block, 0, s, a);
    } else {
        if (p->f32) hipLaunchKernelGGL((tsdf_raycast_kernel<float, double>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((tsdf_raycast_kernel<double, double>), grid, block, 0, s, a);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_cast.e1, s));
    p->t_cast.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    p->last_cast = a, p->cast_views = n_views;
    return PCS_OK;
}

// The bench's separate counting launch: the last pcs_tsdf_raycast over again (its views, settings and mask; none of its outputs is
// touched), writing per pixel the number of samples the march and the normal evaluated.
int pcs_tsdf_raycast_count_samples(pcs_tsdf_volume *p, uint32_t *d_samples, void *stream) {
    const char *who = "pcs_tsdf_raycast_count_samples";
    if (!d_samples) return fail(PCS_ERR_ARG, "%s: d_samples must be given", who);
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (!p->have_grid || p->cast_views == 0) return fail(PCS_ERR_STATE, "%s: no pcs_tsdf_raycast on the volume as it stands", who);
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, false));
    TsdfRaycastArgs a = p->last_cast;
    a.samples = d_samples;
    const dim3 grid((unsigned)((a.W + TSDF_RAY_BLOCK - 1) / TSDF_RAY_BLOCK), (unsigned)((a.H + TSDF_RAY_BLOCK - 1) / TSDF_RAY_BLOCK), (unsigned)p->cast_views),
        block(TSDF_RAY_BLOCK * TSDF_RAY_BLOCK);
    if (p->f32) hipLaunchKernelGGL((tsdf_raycast_kernel<float, float, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((tsdf_raycast_kernel<double, float, true>), grid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

// Device time of the last cast's mask pass (memset and mask kernel) and of its cast kernel; either pointer may be NULL.  PCS_ERR_STATE
// when the part asked for did not run: no cast yet, or a mask asked for after a cast without one.
int pcs_tsdf_raycast_last_kernel_ms(pcs_tsdf_volume *p, float *mask_ms, float *cast_ms) {
    const char *who = "pcs_tsdf_raycast_last_kernel_ms";
    if (!p || (!mask_ms && !cast_ms)) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (mask_ms)
        if (const int rc = timer_ms(who, &p->t_mask, mask_ms, "the last cast made no mask")) return rc;
    if (cast_ms)
        if (const int rc = timer_ms(who, &p->t_cast, cast_ms, "no cast has run yet")) return rc;
    return PCS_OK;
}

// Device time of the last integration, of the last count (classification, numbering, quad flags and both scans) and of the last write;
// any pointer may be NULL.
int pcs_tsdf_last_kernel_ms(pcs_tsdf_volume *p, float *integrate_ms, float *count_ms, float *write_ms) {
    const char *who = "pcs_tsdf_last_kernel_ms";
    if (!p || (!integrate_ms && !count_ms && !write_ms)) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (integrate_ms)
        if (const int rc = timer_ms(who, &p->t_integrate, integrate_ms, "no integration has run yet")) return rc;
    if (count_ms)
        if (const int rc = timer_ms(who, &p->t_count, count_ms, "no count has run yet")) return rc;
    if (write_ms)
        if (const int rc = timer_ms(who, &p->t_write, write_ms, "no write has run yet")) return rc;
    return PCS_OK;
}

}  // extern "C"

// ---- colour of surface points from the images (include/pcs_hip.h, row f19; kernels: ba_tsdf_colour.hpp) -----------------------------------------
static_assert(TSDF_COLOUR_BLEND == PCS_COLOUR_BLEND && TSDF_COLOUR_BEST == PCS_COLOUR_BEST, "modes of pcs_hip.h");

// What both colour entry points take of the source views, the images, the visibility maps, the rule's settings and the outputs.
struct TsdfColourSource {
    int64_t n_views;
    int width, height;
    const double *K, *P;
    const void *d_images;
    int64_t pitch;
    int channels, image_dtype;
    const void *d_visibility;
    int visibility_dtype;
    double occlusion_tol, cos_min;
    int mode;
    const double *fill;
    void *d_colour;
    int colour_dtype;
    float *d_weight;
    uint16_t *d_count;
    int32_t *d_best;
};

// Every argument of the source side: nothing here touches the device.
static int tsdf_check_colour_source(const char *who, const TsdfColourSource &c) {
    if (const int rc = fuse_check_views(who, c.n_views, c.width, c.height, c.K, c.P)) return rc;
    if (c.width < 2 || c.height < 2) return fail(PCS_ERR_ARG, "%s: width %d, height %d: a source image needs both sides >= 2", who, c.width, c.height);
    if (c.channels != 1 && c.channels != 3 && c.channels != 4) return fail(PCS_ERR_ARG, "%s: channels %d (1, 3 or 4)", who, c.channels);
    if (c.image_dtype != PCS_IMAP_U8 && c.image_dtype != PCS_IMAP_F32) return fail(PCS_ERR_ARG, "%s: image_dtype PCS_IMAP_U8 or PCS_IMAP_F32", who);
    const int64_t esz = c.image_dtype == PCS_IMAP_U8 ? 1 : 4;
    if (c.pitch < (int64_t)c.width * c.channels * esz || c.pitch % esz != 0 || c.pitch > ((int64_t)1 << 40))
        return fail(PCS_ERR_ARG, "%s: pitch %lld must be a multiple of the element size, at least width * channels * element size = %lld", who, (long long)c.pitch,
                    (long long)((int64_t)c.width * c.channels * esz));
    if (!c.d_images) return fail(PCS_ERR_ARG, "%s: d_images must be given", who);
    if ((uintptr_t)c.d_images % (uintptr_t)esz != 0) return fail(PCS_ERR_ARG, "%s: d_images is not aligned to its element size", who);
    if (c.d_visibility) {
        if (c.visibility_dtype != PCS_F64 && c.visibility_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: visibility_dtype PCS_F64 or PCS_F32", who);
        if (!std::isfinite(c.occlusion_tol) || !(c.occlusion_tol >= 0.0)) return fail(PCS_ERR_ARG, "%s: occlusion_tol must be finite and >= 0 (got %g)", who, c.occlusion_tol);
    }
    if (!(c.cos_min >= 0.0 && c.cos_min < 1.0)) return fail(PCS_ERR_ARG, "%s: cos_min %g outside [0, 1)", who, c.cos_min);
    if (c.mode != PCS_COLOUR_BLEND && c.mode != PCS_COLOUR_BEST) return fail(PCS_ERR_ARG, "%s: mode PCS_COLOUR_BLEND or PCS_COLOUR_BEST", who);
    for (int k = 0; c.fill && k < c.channels; ++k)
        if (std::isinf(c.fill[k])) return fail(PCS_ERR_ARG, "%s: fill[%d] is infinite", who, k);
    if (c.colour_dtype != PCS_IMAP_U8 && c.colour_dtype != PCS_IMAP_F32) return fail(PCS_ERR_ARG, "%s: colour_dtype PCS_IMAP_U8 or PCS_IMAP_F32", who);
    if (!c.d_colour) return fail(PCS_ERR_ARG, "%s: d_colour must be given", who);
    return PCS_OK;
}

// The table of the source views: per view the 16 doubles of pcs_fuse_set_views, then the centre C of the render rows, then one unused
static std::vector<double> tsdf_colour_rows(int64_t n_views, const double *K, const double *P) {
    const std::vector<double> fuse = fuse_view_rows(n_views, K, P), render = tsdf_render_rows(n_views, K, P);
    std::vector<double> rows(TSDF_COLOUR_ROW * (size_t)n_views, 0.0);
    for (int64_t v = 0; v < n_views; ++v) {
        std::copy(fuse.begin() + 16 * v, fuse.begin() + 16 * v + 16, rows.begin() + TSDF_COLOUR_ROW * v);
        std::copy(render.begin() + 16 * v + 13, render.begin() + 16 * v + 16, rows.begin() + TSDF_COLOUR_ROW * v + 16);
    }
    return rows;
}

static TsdfColourArgs tsdf_colour_args(const pcs_tsdf_volume *p, const TsdfColourSource &c) {
    TsdfColourArgs a{};
    a.views = p->cviews.as<const double>(), a.n_views = (int)c.n_views, a.W = c.width, a.H = c.height, a.images = c.d_images, a.pitch = c.pitch;
    a.vis = c.d_visibility, a.vis_f32 = c.visibility_dtype == PCS_F32, a.tol = c.d_visibility ? c.occlusion_tol : 0.0, a.cos_min = c.cos_min, a.mode = c.mode;
    for (int k = 0; k < 4; ++k) a.fill[k] = c.fill && k < c.channels ? c.fill[k] : 0.0;
    a.colour = c.d_colour, a.colour_f32 = c.colour_dtype == PCS_IMAP_F32, a.weight = c.d_weight, a.count = c.d_count, a.best = c.d_best;
    return a;
}

// One of the 2 x 2 x 3 x 2 x 2 instantiations of either colour kernel.  TP: the points' type, or the depth maps' for the render views.
template <bool VIEWS, class TI, class TP, int C, bool VIS, bool NRM>
static void tsdf_colour_launch5(dim3 grid, dim3 block, hipStream_t s, const TsdfColourArgs &a) {
    if constexpr (VIEWS) hipLaunchKernelGGL((tsdf_colour_views_kernel<TI, TP, C, VIS, NRM>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((tsdf_colour_points_kernel<TI, TP, C, VIS, NRM>), grid, block, 0, s, a);
}
template <bool VIEWS, class TI, class TP, int C>
static void tsdf_colour_launch3(bool vis, bool nrm, dim3 grid, dim3 block, hipStream_t s, const TsdfColourArgs &a) {
    if (vis && nrm) tsdf_colour_launch5<VIEWS, TI, TP, C, true, true>(grid, block, s, a);
    else if (vis) tsdf_colour_launch5<VIEWS, TI, TP, C, true, false>(grid, block, s, a);
    else if (nrm) tsdf_colour_launch5<VIEWS, TI, TP, C, false, true>(grid, block, s, a);
    else tsdf_colour_launch5<VIEWS, TI, TP, C, false, false>(grid, block, s, a);
}
template <bool VIEWS, class TI, class TP>
static void tsdf_colour_launch2(int channels, bool vis, bool nrm, dim3 grid, dim3 block, hipStream_t s, const TsdfColourArgs &a) {
    if (channels == 1) tsdf_colour_launch3<VIEWS, TI, TP, 1>(vis, nrm, grid, block, s, a);
    else if (channels == 3) tsdf_colour_launch3<VIEWS, TI, TP, 3>(vis, nrm, grid, block, s, a);
    else tsdf_colour_launch3<VIEWS, TI, TP, 4>(vis, nrm, grid, block, s, a);
}
template <bool VIEWS>
static void tsdf_colour_launch(bool image_f32, bool point_f32, int channels, bool vis, bool nrm, dim3 grid, dim3 block, hipStream_t s, const TsdfColourArgs &a) {
    if (image_f32 && point_f32) tsdf_colour_launch2<VIEWS, float, float>(channels, vis, nrm, grid, block, s, a);
    else if (image_f32) tsdf_colour_launch2<VIEWS, float, double>(channels, vis, nrm, grid, block, s, a);
    else if (point_f32) tsdf_colour_launch2<VIEWS, uint8_t, float>(channels, vis, nrm, grid, block, s, a);
    else tsdf_colour_launch2<VIEWS, uint8_t, double>(channels, vis, nrm, grid, block, s, a);
}

static int tsdf_check_points(const char *who, int64_t n, const void *d_points, int point_dtype) {
    if (n < 0 || n > (int64_t)INT32_MAX * TSDF_COLOUR_BLOCK) return fail(PCS_ERR_ARG, "%s: n %lld outside [0, %lld]", who, (long long)n, (long long)INT32_MAX * TSDF_COLOUR_BLOCK);
    if (point_dtype != PCS_F64 && point_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: point_dtype PCS_F64 or PCS_F32", who);
    if (n > 0 && !d_points) return fail(PCS_ERR_ARG, "%s: d_points must be given", who);
    return PCS_OK;
}

extern "C" {

// The cast's normal rule at n arbitrary points (mesh vertices): reads the volume only.
int pcs_tsdf_point_normals(pcs_tsdf_volume *p, int64_t n, const void *d_points, int point_dtype, int min_weight, float *d_normals, uint8_t *d_status, void *stream) {
    const char *who = "pcs_tsdf_point_normals";
    if (const int rc = tsdf_check_points(who, n, d_points, point_dtype)) return rc;
    if (min_weight < 1 || min_weight > TSDF_MAX_WEIGHT) return fail(PCS_ERR_ARG, "%s: min_weight %d outside [1, %d]", who, min_weight, TSDF_MAX_WEIGHT);
    if (n > 0 && !d_normals) return fail(PCS_ERR_ARG, "%s: d_normals must be given", who);
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (!p->have_grid) return fail(PCS_ERR_ARG, "%s: no grid: pcs_tsdf_set_grid comes first", who);
    if (n == 0) return PCS_OK;
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, false));
    TsdfPointNormalArgs a{};
    a.field.sum = p->sum.p, a.field.weight = p->weight.as<const uint16_t>(), a.field.g = p->g, a.field.min_weight = min_weight;
    a.n = n, a.points = d_points, a.normals = d_normals, a.status = d_status;
    const dim3 grid((unsigned)((n + TSDF_COLOUR_BLOCK - 1) / TSDF_COLOUR_BLOCK)), block(TSDF_COLOUR_BLOCK);
    HIPCHK(hipEventRecord(p->t_pnormal.e0, s));
    const bool p32 = point_dtype == PCS_F32;
    if (p->f32 && p32) hipLaunchKernelGGL((tsdf_point_normals_kernel<float, float>), grid, block, 0, s, a);
    else if (p->f32) hipLaunchKernelGGL((tsdf_point_normals_kernel<float, double>), grid, block, 0, s, a);
    else if (p32) hipLaunchKernelGGL((tsdf_point_normals_kernel<double, float>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((tsdf_point_normals_kernel<double, double>), grid, block, 0, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_pnormal.e1, s));
    p->t_pnormal.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

// The colour of n caller-supplied points (the rule: include/pcs_hip.h).  K, P and fill are HOST arrays and are copied; the points, the
// normals, the images, the visibility maps and every output are DEVICE buffers.  It needs no grid and leaves the volume, the
// integration's view table, a preceding count and the last cast as they are.
int pcs_tsdf_colour_points(pcs_tsdf_volume *p, int64_t n, const void *d_points, int point_dtype, const float *d_normals, int64_t n_views, int width, int height,
                           const double *K, const double *P, const void *d_images, int64_t pitch, int channels, int image_dtype, const void *d_visibility,
                           int visibility_dtype, double occlusion_tol, double cos_min, int mode, const double *fill, void *d_colour, int colour_dtype, float *d_weight,
                           uint16_t *d_count, int32_t *d_best, void *stream) {
    const char *who = "pcs_tsdf_colour_points";
    const TsdfColourSource c{n_views, width, height, K, P, d_images, pitch, channels, image_dtype, d_visibility, visibility_dtype, occlusion_tol, cos_min, mode, fill,
                             d_colour, colour_dtype, d_weight, d_count, d_best};
    if (const int rc = tsdf_check_points(who, n, d_points, point_dtype)) return rc;
    if (const int rc = tsdf_check_colour_source(who, c)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (n == 0) return PCS_OK;
    const std::vector<double> rows = tsdf_colour_rows(n_views, K, P);
    HIPCHK(p->core.quiesce());   // a queued colour run may still read the old table
    const HostArray up[] = {{p->cviews, rows.data(), TSDF_COLOUR_ROW * n_views, sizeof(double)}};
    if (const int rc = upload_host_arrays(p->core, up, 1)) return rc;
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, false));
    TsdfColourArgs a = tsdf_colour_args(p, c);
    a.n = n, a.points = d_points, a.normals = d_normals;
    const dim3 grid((unsigned)((n + TSDF_COLOUR_BLOCK - 1) / TSDF_COLOUR_BLOCK)), block(TSDF_COLOUR_BLOCK);
    HIPCHK(hipEventRecord(p->t_colour.e0, s));
    tsdf_colour_launch<false>(image_dtype == PCS_IMAP_F32, point_dtype == PCS_F32, channels, d_visibility != nullptr, d_normals != nullptr, grid, block, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_colour.e1, s));
    p->t_colour.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

// The same rule with the pixels of n_render render views as the points: pixel (x, y) at z-depth d_depth is C + z w by the cast's ray
// formulas.  K_render, P_render, K, P and fill are HOST arrays and are copied.  Outputs in image order (n_render, r_height, r_width, ...).
int pcs_tsdf_colour_views(pcs_tsdf_volume *p, int64_t n_render, int r_width, int r_height, const double *K_render, const double *P_render, const void *d_depth,
                          int depth_dtype, const float *d_normal, int64_t n_views, int width, int height, const double *K, const double *P, const void *d_images,
                          int64_t pitch, int channels, int image_dtype, const void *d_visibility, int visibility_dtype, double occlusion_tol, double cos_min, int mode,
                          const double *fill, void *d_colour, int colour_dtype, float *d_weight, uint16_t *d_count, int32_t *d_best, void *stream) {
    const char *who = "pcs_tsdf_colour_views";
    const TsdfColourSource c{n_views, width, height, K, P, d_images, pitch, channels, image_dtype, d_visibility, visibility_dtype, occlusion_tol, cos_min, mode, fill,
                             d_colour, colour_dtype, d_weight, d_count, d_best};
    if (!K_render || !P_render) return fail(PCS_ERR_ARG, "%s: K_render (n_render, 4) and P_render (n_render, 12) must be given", who);
    if (const int rc = fuse_check_views(who, n_render, r_width, r_height, K_render, P_render)) return rc;
    if (n_render > 65535) return fail(PCS_ERR_ARG, "%s: n_render %lld above 65535", who, (long long)n_render);
    if (depth_dtype != PCS_F64 && depth_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: depth_dtype PCS_F64 or PCS_F32", who);
    if (!d_depth) return fail(PCS_ERR_ARG, "%s: d_depth must be given", who);
    if (const int rc = tsdf_check_colour_source(who, c)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    const std::vector<double> rows = tsdf_colour_rows(n_views, K, P), rrows = tsdf_render_rows(n_render, K_render, P_render);
    HIPCHK(p->core.quiesce());
    const HostArray up[] = {{p->cviews, rows.data(), TSDF_COLOUR_ROW * n_views, sizeof(double)}, {p->crviews, rrows.data(), 16 * n_render, sizeof(double)}};
    if (const int rc = upload_host_arrays(p->core, up, 2)) return rc;
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, false));
    TsdfColourArgs a = tsdf_colour_args(p, c);
    a.n = (int64_t)n_render * r_height * r_width, a.normals = d_normal, a.rviews = p->crviews.as<const double>(), a.depth = d_depth, a.RW = r_width, a.RH = r_height;
    const dim3 grid((unsigned)((r_width + TSDF_RAY_BLOCK - 1) / TSDF_RAY_BLOCK), (unsigned)((r_height + TSDF_RAY_BLOCK - 1) / TSDF_RAY_BLOCK), (unsigned)n_render),
        block(TSDF_RAY_BLOCK * TSDF_RAY_BLOCK);
    HIPCHK(hipEventRecord(p->t_colour.e0, s));
    tsdf_colour_launch<true>(image_dtype == PCS_IMAP_F32, depth_dtype == PCS_F32, channels, d_visibility != nullptr, d_normal != nullptr, grid, block, s, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->t_colour.e1, s));
    p->t_colour.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

// Device time of the last pcs_tsdf_point_normals and of the last colour kernel (points or views); either pointer may be NULL.
int pcs_tsdf_colour_last_kernel_ms(pcs_tsdf_volume *p, float *normals_ms, float *colour_ms) {
    const char *who = "pcs_tsdf_colour_last_kernel_ms";
    if (!p || (!normals_ms && !colour_ms)) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (normals_ms)
        if (const int rc = timer_ms(who, &p->t_pnormal, normals_ms, "no point normals have run yet")) return rc;
    if (colour_ms)
        if (const int rc = timer_ms(who, &p->t_colour, colour_ms, "no colour kernel has run yet")) return rc;
    return PCS_OK;
}

}  // extern "C"
