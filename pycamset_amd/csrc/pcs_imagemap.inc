// pcs_imagemap.inc — host side of the image mapper (included by pcs_engine.hip; kernels: ba_imagemap.hpp).  The handle owns the camera
// table and the per-image camera indices of the last remap; points, maps and images are the caller's device buffers.  Fence and
// timer are those of pcs_handle.inc (DESIGN.md, "Batched handles").
struct pcs_image_mapper {
    HandleCore core;
    KernelTimer timer;
    DevBuf tab, cams;
    int64_t n_cams = -1;            // -1: cameras not set
    bool have_ext = false;
    std::vector<double> h_tab;      // the table as uploaded: set_view rewrites its view columns
    std::vector<int32_t> h_cams;    // the indices p->cams holds (a run of frames with the same cameras uploads them once)
};

static int imap_upload_table(pcs_image_mapper *p, const std::vector<double> &tab, int64_t n_cams) {
    HIPCHK(p->core.quiesce());   // a run queued on any stream may still read the table
    if (const int rc = p->tab.grow(n_cams * IMAP_CAM_STRIDE, sizeof(double))) return rc;
    HIPCHK(hipMemcpy(p->tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    return PCS_OK;
}

static bool imap_focal_ok(double fx, double fy) { return std::isfinite(fx) && std::isfinite(fy) && fx != 0.0 && fy != 0.0; }

static_assert(IMAP_MODE_UNDISTORT == PCS_IMAP_UNDISTORT && IMAP_MODE_DISTORT == PCS_IMAP_DISTORT && IMAP_MODE_RAY == PCS_IMAP_RAY &&
              IMAP_NORMALISED == PCS_IMAP_NORMALISED && IMAP_WORLD == PCS_IMAP_WORLD && IMAP_NO_DISTORT == PCS_IMAP_NO_DISTORT &&
              IMAP_NEAREST == PCS_IMAP_NEAREST && IMAP_BILINEAR == PCS_IMAP_BILINEAR && IMAP_BICUBIC == PCS_IMAP_BICUBIC, "codes of pcs_hip.h");
constexpr int IMAP_MAX_ITERS = 100;
constexpr int IMAP_RAY_FLAGS = PCS_IMAP_NORMALISED | PCS_IMAP_WORLD | PCS_IMAP_NO_DISTORT;

static int imap_check_ray_options(const char *who, const pcs_image_mapper *p, int flags, int iters) {
    if (flags & ~IMAP_RAY_FLAGS) return fail(PCS_ERR_ARG, "%s: unknown flags %d", who, flags);
    if (iters < 0 || iters > IMAP_MAX_ITERS) return fail(PCS_ERR_ARG, "%s: iters %d outside [0, %d]", who, iters, IMAP_MAX_ITERS);
    if ((flags & PCS_IMAP_WORLD) && !p->have_ext) return fail(PCS_ERR_STATE, "%s: PCS_IMAP_WORLD needs the ext of pcs_imap_set_cameras", who);
    return PCS_OK;
}

// what every launch shares: the fence in front, the timer around, the fence behind
template <class Launch>
static int imap_run(pcs_image_mapper *p, void *stream, bool grows, Launch launch) {
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));
    HIPCHK(hipEventRecord(p->timer.e0, s));
    launch(s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->timer.e1, s));
    p->timer.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

static int imap_check_plane(const char *who, const pcs_image_mapper *p, int cam, int width, int height, const void *d_out, int out_dtype) {
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (p->n_cams < 0) return fail(PCS_ERR_STATE, "%s: cameras not set", who);
    if (cam < 0 || cam >= p->n_cams) return fail(PCS_ERR_ARG, "%s: cam %d outside [0, %lld)", who, cam, (long long)p->n_cams);
    if (width < 1 || height < 1 || (int64_t)width * height > (int64_t)INT32_MAX * 128) return fail(PCS_ERR_ARG, "%s: width %d, height %d: both must be >= 1", who, width, height);
    if (!d_out || (out_dtype != PCS_F64 && out_dtype != PCS_F32)) return fail(PCS_ERR_ARG, "%s: d_out with out_dtype PCS_F64 or PCS_F32", who);
    return PCS_OK;
}

template <class T, int C>
static void imap_launch_remap(int interpolation, dim3 grid, hipStream_t s, const ImapRemapArgs &a) {
    const dim3 block(IMAP_TILE_X, IMAP_TILE_Y);
    if (interpolation == PCS_IMAP_NEAREST) hipLaunchKernelGGL((imap_remap_kernel<T, C, IMAP_NEAREST>), grid, block, 0, s, a);
    else if (interpolation == PCS_IMAP_BILINEAR) hipLaunchKernelGGL((imap_remap_kernel<T, C, IMAP_BILINEAR>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((imap_remap_kernel<T, C, IMAP_BICUBIC>), grid, block, 0, s, a);
}

template <class T>
static void imap_launch_remap_channels(int channels, int interpolation, dim3 grid, hipStream_t s, const ImapRemapArgs &a) {
    if (channels == 1) imap_launch_remap<T, 1>(interpolation, grid, s, a);
    else if (channels == 3) imap_launch_remap<T, 3>(interpolation, grid, s, a);
    else imap_launch_remap<T, 4>(interpolation, grid, s, a);
}

extern "C" {
int pcs_imap_create(pcs_image_mapper **out, int device) {
    if (!out) return fail(PCS_ERR_ARG, "pcs_imap_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_imap_create", device)) return rc;
    pcs_image_mapper *p = new pcs_image_mapper();
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->timer.create();
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_imap_create: %s", hipGetErrorString(e));
        pcs_imap_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_imap_destroy(pcs_image_mapper *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->tab, &p->cams}, {&p->timer});
    delete p;
    return PCS_OK;
}

// Everything is checked on the host before anything changes: a refused call keeps the previous cameras.  Resets the view.
int pcs_imap_set_cameras(pcs_image_mapper *p, int64_t n_cams, const double *intr, const double *ext) {
    const char *who = "pcs_imap_set_cameras";
    if (!p || !intr || n_cams < 1 || n_cams > (1 << 20)) return fail(PCS_ERR_ARG, "%s: bad arguments (a handle, intr (n_cams, 9), 1 <= n_cams <= 2^20)", who);
    for (int64_t c = 0; c < n_cams; ++c) {
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(intr[9 * c + k])) return fail(PCS_ERR_ARG, "%s: intr of camera %lld is not finite", who, (long long)c);
        if (!imap_focal_ok(intr[9 * c], intr[9 * c + 2])) return fail(PCS_ERR_ARG, "%s: intr of camera %lld has a focal length of 0", who, (long long)c);
        for (int k = 0; ext && k < 12; ++k)
            if (!std::isfinite(ext[12 * c + k])) return fail(PCS_ERR_ARG, "%s: ext of camera %lld is not finite", who, (long long)c);
    }
    std::vector<double> tab((size_t)n_cams * IMAP_CAM_STRIDE, 0.0);
    for (int64_t c = 0; c < n_cams; ++c) {
        double *ct = tab.data() + c * IMAP_CAM_STRIDE;
        const double I34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        const double *E = ext ? ext + 12 * c : I34;
        for (int k = 0; k < 12; ++k) ct[IMAP_EXT + k] = E[k];
        for (int k = 0; k < 3; ++k) ct[IMAP_POS + k] = ext ? -(E[k] * E[3] + E[4 + k] * E[7] + E[8 + k] * E[11]) : 0.0;   // -R^T t
        for (int k = 0; k < 9; ++k) ct[IMAP_INTR + k] = intr[9 * c + k];
        for (int k = 0; k < 9; ++k) ct[IMAP_VIEW + k] = (k % 4 == 0) ? 1.0 : 0.0;
        for (int k = 0; k < 4; ++k) ct[IMAP_KNEW + k] = intr[9 * c + k];
    }
    if (const int rc = imap_upload_table(p, tab, n_cams)) return rc;
    p->h_tab.swap(tab);
    p->n_cams = n_cams;
    p->have_ext = ext != nullptr;
    return PCS_OK;
}

// The view of every camera for build_maps and the fused remap: R_new (n_cams, 9) row-major or NULL = identity, K_new (n_cams, 4) =
// [fx, cx, fy, cy] or NULL = the camera's own.  A refused call keeps the previous view.
int pcs_imap_set_view(pcs_image_mapper *p, const double *R_new, const double *K_new) {
    const char *who = "pcs_imap_set_view";
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (p->n_cams < 0) return fail(PCS_ERR_STATE, "%s: cameras not set", who);
    for (int64_t c = 0; c < p->n_cams; ++c) {
        for (int k = 0; R_new && k < 9; ++k)
            if (!std::isfinite(R_new[9 * c + k])) return fail(PCS_ERR_ARG, "%s: R_new of camera %lld is not finite", who, (long long)c);
        if (K_new) {
            for (int k = 0; k < 4; ++k)
                if (!std::isfinite(K_new[4 * c + k])) return fail(PCS_ERR_ARG, "%s: K_new of camera %lld is not finite", who, (long long)c);
            if (!imap_focal_ok(K_new[4 * c], K_new[4 * c + 2])) return fail(PCS_ERR_ARG, "%s: K_new of camera %lld has a focal length of 0", who, (long long)c);
        }
    }
    std::vector<double> tab = p->h_tab;
    for (int64_t c = 0; c < p->n_cams; ++c) {
        double *ct = tab.data() + c * IMAP_CAM_STRIDE;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) ct[IMAP_VIEW + 3 * i + j] = R_new ? R_new[9 * c + 3 * j + i] : (i == j ? 1.0 : 0.0);   // V = R_new^T
        for (int k = 0; k < 4; ++k) ct[IMAP_KNEW + k] = K_new ? K_new[4 * c + k] : ct[IMAP_INTR + k];
    }
    if (const int rc = imap_upload_table(p, tab, p->n_cams)) return rc;
    p->h_tab.swap(tab);
    return PCS_OK;
}

int pcs_imap_points(pcs_image_mapper *p, int mode, int64_t n, const int32_t *d_cam, int cam_all, const double *d_in, int iters, int flags, double *d_out, void *stream) {
    const char *who = "pcs_imap_points";
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (p->n_cams < 0) return fail(PCS_ERR_STATE, "%s: cameras not set", who);
    if (mode < PCS_IMAP_UNDISTORT || mode > PCS_IMAP_RAY) return fail(PCS_ERR_ARG, "%s: mode %d is none of PCS_IMAP_UNDISTORT, PCS_IMAP_DISTORT, PCS_IMAP_RAY", who, mode);
    if (n < 0 || n > (int64_t)INT32_MAX * 256 || (n > 0 && (!d_in || !d_out))) return fail(PCS_ERR_ARG, "%s: bad arguments (n >= 0, d_in (n, 2), d_out)", who);
    if (!d_cam && (cam_all < 0 || cam_all >= p->n_cams)) return fail(PCS_ERR_ARG, "%s: cam_all %d outside [0, %lld)", who, cam_all, (long long)p->n_cams);
    if (const int rc = imap_check_ray_options(who, p, mode == PCS_IMAP_RAY ? flags : 0, iters)) return rc;
    if (mode != PCS_IMAP_RAY && flags != 0) return fail(PCS_ERR_ARG, "%s: flags go with PCS_IMAP_RAY", who);
    if (n == 0) return PCS_OK;
    return imap_run(p, stream, false, [&](hipStream_t s) {
        hipLaunchKernelGGL(imap_points_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p->tab.as<const double>(), (int)p->n_cams, mode, n, d_cam, cam_all,
                           reinterpret_cast<const double2 *>(d_in), iters, flags, d_out);
    });
}

int pcs_imap_rays(pcs_image_mapper *p, int cam, int width, int height, int flags, int iters, const void *d_depth, int depth_dtype, void *d_out, int out_dtype, void *stream) {
    const char *who = "pcs_imap_rays";
    if (const int rc = imap_check_plane(who, p, cam, width, height, d_out, out_dtype)) return rc;
    if (const int rc = imap_check_ray_options(who, p, flags, iters)) return rc;
    if (d_depth && depth_dtype != PCS_F64 && depth_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: depth_dtype PCS_F64 or PCS_F32", who);
    const dim3 grid((unsigned)(((int64_t)width * height + 255) / 256));
    return imap_run(p, stream, false, [&](hipStream_t s) {
        if (out_dtype == PCS_F32)
            hipLaunchKernelGGL(imap_raymap_kernel<float>, grid, dim3(256), 0, s, p->tab.as<const double>(), cam, width, height, flags, iters, d_depth, depth_dtype == PCS_F32,
                               static_cast<float *>(d_out));
        else
            hipLaunchKernelGGL(imap_raymap_kernel<double>, grid, dim3(256), 0, s, p->tab.as<const double>(), cam, width, height, flags, iters, d_depth, depth_dtype == PCS_F32,
                               static_cast<double *>(d_out));
    });
}

int pcs_imap_build_maps(pcs_image_mapper *p, int cam, int width, int height, void *d_out, int out_dtype, void *stream) {
    if (const int rc = imap_check_plane("pcs_imap_build_maps", p, cam, width, height, d_out, out_dtype)) return rc;
    const dim3 grid((unsigned)(((int64_t)width * height + 255) / 256));
    return imap_run(p, stream, false, [&](hipStream_t s) {
        if (out_dtype == PCS_F32) hipLaunchKernelGGL(imap_build_maps_kernel<float>, grid, dim3(256), 0, s, p->tab.as<const double>(), cam, width, height, static_cast<float *>(d_out));
        else hipLaunchKernelGGL(imap_build_maps_kernel<double>, grid, dim3(256), 0, s, p->tab.as<const double>(), cam, width, height, static_cast<double *>(d_out));
    });
}

// Every argument is checked on the host before the device is touched.  `cams` is a HOST array: it is range-checked here, which keeps
// the kernel's table and map reads inside their buffers.
int pcs_imap_remap(pcs_image_mapper *p, int64_t n_img, const int32_t *cams, const void *d_src, int src_width, int src_height, int channels, int dtype, int64_t src_pitch,
                   void *d_dst, int dst_width, int dst_height, int64_t dst_pitch, const void *d_map, int map_dtype, int64_t n_maps, int interpolation, const double *border,
                   uint8_t *d_valid, void *stream) {
    const char *who = "pcs_imap_remap";
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (n_img < 0 || n_img > 65535) return fail(PCS_ERR_ARG, "%s: n_img %lld outside [0, 65535]", who, (long long)n_img);
    if (n_img > 0 && (!cams || !d_src || !d_dst)) return fail(PCS_ERR_ARG, "%s: cams, d_src and d_dst must be given", who);
    if (channels != 1 && channels != 3 && channels != 4) return fail(PCS_ERR_ARG, "%s: channels %d is none of 1, 3, 4", who, channels);
    if (dtype != PCS_IMAP_U8 && dtype != PCS_IMAP_F32) return fail(PCS_ERR_ARG, "%s: dtype %d is neither PCS_IMAP_U8 nor PCS_IMAP_F32", who, dtype);
    if (interpolation < PCS_IMAP_NEAREST || interpolation > PCS_IMAP_BICUBIC)
        return fail(PCS_ERR_ARG, "%s: interpolation %d is none of PCS_IMAP_NEAREST, PCS_IMAP_BILINEAR, PCS_IMAP_BICUBIC", who, interpolation);
    const int64_t elem = dtype == PCS_IMAP_U8 ? 1 : 4;
    if (src_width < 1 || src_height < 1 || dst_width < 1 || dst_height < 1 || src_width > (1 << 24) || src_height > (1 << 24) || dst_width > (1 << 24) || dst_height > 65535 * IMAP_TILE_Y)
        return fail(PCS_ERR_ARG, "%s: image sizes must be >= 1 (at most 2^24; dst_height at most %d)", who, 65535 * IMAP_TILE_Y);
    if (src_pitch < src_width * channels * elem) return fail(PCS_ERR_ARG, "%s: src_pitch %lld below the row size %lld", who, (long long)src_pitch, (long long)(src_width * channels * elem));
    if (dst_pitch < dst_width * channels * elem) return fail(PCS_ERR_ARG, "%s: dst_pitch %lld below the row size %lld", who, (long long)dst_pitch, (long long)(dst_width * channels * elem));
    if (elem == 4 && (src_pitch % 4 || dst_pitch % 4 || ((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 3)))
        return fail(PCS_ERR_ARG, "%s: float images need 4-byte aligned buffers and pitches (src_pitch, dst_pitch)", who);
    if (d_map) {
        if (map_dtype != PCS_F64 && map_dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: map_dtype PCS_F64 or PCS_F32", who);
        if (n_maps < 1) return fail(PCS_ERR_ARG, "%s: n_maps must be >= 1 with a map", who);
        if (((uintptr_t)d_map & (map_dtype == PCS_F64 ? 7 : 3))) return fail(PCS_ERR_ARG, "%s: d_map is not aligned to its element", who);
    } else if (p->n_cams < 0) {
        return fail(PCS_ERR_STATE, "%s: cameras not set (the fused form computes the coordinates from them)", who);
    }
    const int64_t limit = d_map ? n_maps : p->n_cams;
    for (int64_t i = 0; i < n_img; ++i)
        if (cams[i] < 0 || cams[i] >= limit) return fail(PCS_ERR_ARG, "%s: cams[%lld] = %d outside [0, %lld)", who, (long long)i, cams[i], (long long)limit);
    if (n_img == 0) return PCS_OK;
    ImapRemapArgs a;
    a.src = d_src, a.dst = d_dst, a.valid = d_valid, a.map = d_map;
    a.coord = !d_map ? IMAP_COORD_FUSED : map_dtype == PCS_F32 ? IMAP_COORD_MAP_F32 : IMAP_COORD_MAP_F64;
    a.Ws = src_width, a.Hs = src_height, a.Wd = dst_width, a.Hd = dst_height, a.src_pitch = src_pitch, a.dst_pitch = dst_pitch;
    for (int c = 0; c < 4; ++c) {   // the border as a value of the image's own type
        const double b = border && c < channels ? border[c] : 0.0;
        a.border.v[c] = dtype == PCS_IMAP_U8 ? std::fmin(std::fmax(std::nearbyint(b), 0.0), 255.0) : (double)(float)b;
        if (dtype == PCS_IMAP_U8 && !(b == b)) a.border.v[c] = 0.0;
    }
    // the indices: uploaded when they differ from the ones the handle holds (frame after frame they do not)
    if (p->h_cams.size() != (size_t)n_img || !std::equal(p->h_cams.begin(), p->h_cams.end(), cams)) {
        HIPCHK(p->core.quiesce());   // a queued remap may still read the old ones
        p->h_cams.clear();
        if (const int rc = p->cams.grow(n_img, sizeof(int32_t))) return rc;
        HIPCHK(hipMemcpy(p->cams.p, cams, sizeof(int32_t) * (size_t)n_img, hipMemcpyHostToDevice));
        p->h_cams.assign(cams, cams + n_img);
    }
    a.cams = p->cams.as<const int32_t>(), a.tab = p->tab.as<const double>();
    const dim3 grid((unsigned)((dst_width + IMAP_TILE_X * IMAP_PX - 1) / (IMAP_TILE_X * IMAP_PX)), (unsigned)((dst_height + IMAP_TILE_Y - 1) / IMAP_TILE_Y), (unsigned)n_img);
    return imap_run(p, stream, false, [&](hipStream_t s) {
        if (dtype == PCS_IMAP_U8) imap_launch_remap_channels<uint8_t>(channels, interpolation, grid, s, a);
        else imap_launch_remap_channels<float>(channels, interpolation, grid, s, a);
    });
}

// Device time of the last launch of this handle (points, rays, build_maps or remap).
int pcs_imap_last_kernel_ms(pcs_image_mapper *p, float *kernel_ms) {
    return timer_ms("pcs_imap_last_kernel_ms", p ? &p->timer : nullptr, kernel_ms, "nothing has run yet");
}

}  // extern "C"
