// pcs_stereo.inc — host side of the stereo matchers (included by pcs_engine.hip; kernels: ba_stereo.hpp, ba_stereo_sgm.hpp).  The handle
// owns the workspace: the two prefiltered planes, the right-anchored disparity, the compaction's block counts and offsets, and the Q / T
// matrices of the last reprojection — O(n H W) bytes, never the matching-cost volume — and, once pcs_stereo_sgm has run, the aggregated
// volume S and the census planes of one chunk of pairs, under the limit of pcs_stereo_set_sgm_workspace.  Images, disparities and points are the caller's device buffers.  Fence
// and timer are those of pcs_handle.inc (DESIGN.md, "Batched handles").
struct pcs_stereo_matcher {
    HandleCore core;
    KernelTimer timer;
    DevBuf planes, dr, blk, off, qt;   // planes: uint8 (2, n, H, W); dr: int16 (n, H, W); blk: int32 (NB); off: int64 (NB + 1); qt: double (12 + 16 n_Q)
    std::vector<double> h_qt;          // what qt holds (the same Q frame after frame is uploaded once)
    DevBuf sgm;                        // pcs_stereo_sgm: [S uint16 (nc, H, W, Dpad)] [descriptors uint64 (2, nc, H, W)] of one chunk of nc pairs
    int64_t sgm_limit = 0;             // bytes sgm may take; 0: SGM_DEFAULT_WORKSPACE
};

static_assert(STEREO_NOT_STRICT == PCS_STEREO_NOT_STRICT && STEREO_TEXTURE == PCS_STEREO_TEXTURE && STEREO_UNIQUENESS == PCS_STEREO_UNIQUENESS &&
              STEREO_LEFT_RIGHT == PCS_STEREO_LEFT_RIGHT && STEREO_VALIDITY == PCS_STEREO_VALIDITY, "status bits of pcs_hip.h");
constexpr int64_t STEREO_MAX_PAIRS = 32767;    // two planes per pair in blockIdx.z of the prefilter
constexpr int STEREO_MAX_SIDE = 65535;         // rows in blockIdx.y
constexpr int64_t STEREO_LDS_LIMIT = 144 * 1024, STEREO_LDS_CU = 160 * 1024;
constexpr int STEREO_WAVES_ENOUGH = 16;          // waves per CU beyond which the model below sees no gain (four per SIMD)
constexpr int64_t STEREO_WORKGROUPS_WANTED = 16384;   // 256 CUs x 16 waves x 4 rounds
constexpr int STEREO_MIN_STRIP = 32;

// The matcher's tiling: K registers of disparities per lane, a tile of TW anchor columns, strips of SH rows.
//   TW  A workgroup is one wave and its column sums take 2 (TW + 2r) Dpad bytes of LDS, so TW decides how many waves a CU holds:
//       the kernel is bound by instruction issue with fewer waves than SIMDs, while a narrow tile spends its time on the 2r halo
//       columns.  TW maximises min(waves per CU, STEREO_WAVES_ENOUGH) * TW / (TW + 2r); ties go to the wider tile.
//   SH  the longest strip that still gives the device STEREO_WORKGROUPS_WANTED one-wave workgroups (a long strip amortises the 2r rows
//       that fill its first window; too few workgroups leave SIMDs without a wave), at least STEREO_MIN_STRIP rows.
// PCS_STEREO_TILE_COLUMNS / PCS_STEREO_STRIP_ROWS in the environment override both (measurements, and the tests of "any tiling gives
// the same bits"); a tile that does not fit the LDS is narrowed until it does.
struct StereoTiling {
    int r, K, Dpad, TW, SH;
    int xs0, xs1, ys0, ys1;   // the strict rectangle (ends exclusive)
    int xr0, xr1;             // anchor columns of the right-anchored pass
    int64_t lds;
};

static int stereo_tile_columns(int r, int Dpad, int wanted) {
    if (wanted > 0) {
        int tw = std::min(wanted, STEREO_MAX_TW);
        while (tw > 1 && stereo_lds_bytes(tw, r, Dpad) > STEREO_LDS_LIMIT) --tw;
        return tw;
    }
    int best = 1;
    double best_score = -1.0;
    for (int tw = 1; tw <= STEREO_MAX_TW; ++tw) {
        const int64_t lds = stereo_lds_bytes(tw, r, Dpad);
        if (lds > STEREO_LDS_LIMIT) break;
        const double score = (double)std::min<int64_t>(STEREO_LDS_CU / lds, STEREO_WAVES_ENOUGH) * tw / (tw + 2 * r);
        if (score >= best_score) best = tw, best_score = score;
    }
    return best;
}

static int stereo_strip_rows(int64_t n, int cols, int rows, int TW) {
    const int64_t tiles_x = (cols + TW - 1) / TW;
    for (int sh = 256; sh > STEREO_MIN_STRIP; sh >>= 1)
        if (tiles_x * ((rows + sh - 1) / sh) * n >= STEREO_WORKGROUPS_WANTED) return sh;
    return STEREO_MIN_STRIP;
}

static int stereo_env_int(const char *name, int lo, int hi) {
    const char *v = std::getenv(name);
    if (!v || !*v) return 0;
    const long x = std::strtol(v, nullptr, 10);
    return x < lo ? 0 : (int)std::min<long>(x, hi);
}

static StereoTiling stereo_tiling(int64_t n, int W, int H, int min_disp, int D, int block, int want_tw = 0, int want_sh = 0) {
    StereoTiling t{};
    t.r = block / 2;
    t.K = 1;
    while (64 * t.K < D) t.K *= 2;
    t.Dpad = 64 * t.K;
    t.TW = stereo_tile_columns(t.r, t.Dpad, want_tw);
    t.lds = stereo_lds_bytes(t.TW, t.r, t.Dpad);
    const int dmax = min_disp + D - 1;
    t.xs0 = t.r + std::max(dmax, 0), t.xs1 = W - t.r + std::min(min_disp, 0);
    t.ys0 = t.r, t.ys1 = H - t.r;
    t.xr0 = t.r, t.xr1 = W - t.r;
    if (t.ys1 < t.ys0) t.ys1 = t.ys0;
    if (t.xs1 < t.xs0) t.xs1 = t.xs0;
    if (t.xr1 < t.xr0) t.xr1 = t.xr0;
    t.SH = want_sh > 0 ? want_sh : stereo_strip_rows(std::max<int64_t>(n, 1), std::max(t.xs1 - t.xs0, 1), std::max(t.ys1 - t.ys0, 1), t.TW);
    return t;
}

// bytes of workspace a match of this shape needs: two planes and the right-anchored disparity
static int64_t stereo_match_workspace(int64_t n, int W, int H) { return n * H * W * (2 + (int64_t)sizeof(int16_t)); }
static int64_t stereo_blocks_per_pair(int W, int H) { return ((int64_t)W * H + STEREO_PIX_PER_BLOCK - 1) / STEREO_PIX_PER_BLOCK; }

static int stereo_check_shape(const char *who, int64_t n, int width, int height) {
    if (n < 0 || n > STEREO_MAX_PAIRS) return fail(PCS_ERR_ARG, "%s: n %lld outside [0, %lld]", who, (long long)n, (long long)STEREO_MAX_PAIRS);
    if (width < 1 || width > STEREO_MAX_SIDE) return fail(PCS_ERR_ARG, "%s: width %d outside [1, %d]", who, width, STEREO_MAX_SIDE);
    if (height < 1 || height > STEREO_MAX_SIDE) return fail(PCS_ERR_ARG, "%s: height %d outside [1, %d]", who, height, STEREO_MAX_SIDE);
    return PCS_OK;
}

// Every argument of pcs_stereo_match but the handle: nothing here touches the device.
static int stereo_check_match(const char *who, int64_t n, int width, int height, const void *d_left, int64_t left_pitch, const void *d_right, int64_t right_pitch, int min_disp,
                              int num_disp, int block, int prefilter_cap, int texture_threshold, int uniqueness_ratio, int lr_max_diff, const void *d_valid_left,
                              const void *d_valid_right, const void *d_disp) {
    if (const int rc = stereo_check_shape(who, n, width, height)) return rc;
    if (min_disp < -STEREO_MAX_DISP || min_disp > STEREO_MAX_DISP) return fail(PCS_ERR_ARG, "%s: min_disp %d outside [-%d, %d]", who, min_disp, STEREO_MAX_DISP, STEREO_MAX_DISP);
    if (num_disp < 1 || num_disp > STEREO_MAX_DISP) return fail(PCS_ERR_ARG, "%s: num_disp %d outside [1, %d]", who, num_disp, STEREO_MAX_DISP);
    if (block < 3 || block > STEREO_MAX_BLOCK || block % 2 == 0) return fail(PCS_ERR_ARG, "%s: block %d must be odd and in [3, %d]", who, block, STEREO_MAX_BLOCK);
    if (prefilter_cap < 0 || prefilter_cap > STEREO_MAX_CAP) return fail(PCS_ERR_ARG, "%s: prefilter_cap %d outside [0, %d]", who, prefilter_cap, STEREO_MAX_CAP);
    if (texture_threshold < 0) return fail(PCS_ERR_ARG, "%s: texture_threshold %d must be >= 0", who, texture_threshold);
    if (prefilter_cap == 0 && texture_threshold != 0) return fail(PCS_ERR_ARG, "%s: texture_threshold %d needs a prefilter_cap > 0 (the texture is measured about the cap)", who, texture_threshold);
    if (uniqueness_ratio < 0 || uniqueness_ratio > 100) return fail(PCS_ERR_ARG, "%s: uniqueness_ratio %d outside [0, 100]", who, uniqueness_ratio);
    if (lr_max_diff < -1) return fail(PCS_ERR_ARG, "%s: lr_max_diff %d must be >= -1 (-1: no left-right check)", who, lr_max_diff);
    if (left_pitch < width) return fail(PCS_ERR_ARG, "%s: left_pitch %lld below the row size %d", who, (long long)left_pitch, width);
    if (right_pitch < width) return fail(PCS_ERR_ARG, "%s: right_pitch %lld below the row size %d", who, (long long)right_pitch, width);
    if ((d_valid_left == nullptr) != (d_valid_right == nullptr)) return fail(PCS_ERR_ARG, "%s: d_valid_left and d_valid_right come together", who);
    if (n > 0 && (!d_left || !d_right)) return fail(PCS_ERR_ARG, "%s: d_left and d_right (the images) must be given", who);
    if (n > 0 && !d_disp) return fail(PCS_ERR_ARG, "%s: d_disp must be given", who);
    return PCS_OK;
}

static int stereo_check_reproject(const char *who, int64_t n, int width, int height, const void *d_disp, const double *Q, int64_t n_Q, double z_lo, double z_hi, const double *T,
                                  const void *d_points, int dtype, const void *d_mask) {
    if (const int rc = stereo_check_shape(who, n, width, height)) return rc;
    if (!Q || (n_Q != 1 && n_Q != n)) return fail(PCS_ERR_ARG, "%s: Q (n_Q, 16) with n_Q = 1 or n (got n_Q %lld for n %lld)", who, (long long)n_Q, (long long)n);
    for (int64_t k = 0; k < 16 * n_Q; ++k)
        if (!std::isfinite(Q[k])) return fail(PCS_ERR_ARG, "%s: Q of pair %lld is not finite", who, (long long)(k / 16));
    for (int k = 0; T && k < 12; ++k)
        if (!std::isfinite(T[k])) return fail(PCS_ERR_ARG, "%s: T is not finite", who);
    if (z_lo != z_lo || z_hi != z_hi) return fail(PCS_ERR_ARG, "%s: z_lo / z_hi must not be NaN (-inf / +inf: no bound)", who);
    if (dtype != PCS_F64 && dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: dtype PCS_F64 or PCS_F32", who);
    if (n > 0 && (!d_disp || !d_points || !d_mask)) return fail(PCS_ERR_ARG, "%s: d_disp, d_points and d_mask must be given", who);
    return PCS_OK;
}

static int stereo_check_compact(const char *who, int64_t n, int width, int height, const void *d_points, int dtype, const void *d_mask, const void *d_values, int64_t values_pitch,
                                const void *d_out_points, const void *d_out_values, const void *d_counts) {
    if (const int rc = stereo_check_shape(who, n, width, height)) return rc;
    if (dtype != PCS_F64 && dtype != PCS_F32) return fail(PCS_ERR_ARG, "%s: dtype PCS_F64 or PCS_F32", who);
    if ((d_values == nullptr) != (d_out_values == nullptr)) return fail(PCS_ERR_ARG, "%s: d_values and d_out_values come together", who);
    if (d_values && values_pitch < width) return fail(PCS_ERR_ARG, "%s: values_pitch %lld below the row size %d", who, (long long)values_pitch, width);
    if (n > 0 && (!d_points || !d_mask || !d_out_points || !d_counts)) return fail(PCS_ERR_ARG, "%s: d_points, d_mask, d_out_points and d_counts must be given", who);
    return PCS_OK;
}

// what every call shares: the fence in front, the workspace, the timer around, the fence behind.  `prepare` grows buffers (it runs behind
// the fence, which has waited on the host when one of them grows), `launch` queues the kernels.
template <class Prepare, class Launch>
static int stereo_run(pcs_stereo_matcher *p, void *stream, bool grows, Prepare prepare, Launch launch) {
    HIPCHK(hipSetDevice(p->core.device));
    hipStream_t s = p->core.stream_or(stream);
    HIPCHK(p->core.fence.before_run(s, grows));
    if (const int rc = prepare()) return rc;
    HIPCHK(hipEventRecord(p->timer.e0, s));
    if (const int rc = launch(s)) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(p->timer.e1, s));
    p->timer.timed = true;
    HIPCHK(p->core.fence.after_run(s));
    return PCS_OK;
}

template <bool RIGHT, int K>
static int stereo_launch_match_k(const StereoMatchArgs &a, dim3 grid, int64_t lds, hipStream_t s) {
    auto kern = stereo_match_kernel<RIGHT, K>;
    if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(64), (std::uint32_t)lds, s, a);
    return PCS_OK;
}

template <bool RIGHT>
static int stereo_launch_match(int K, const StereoMatchArgs &a, dim3 grid, int64_t lds, hipStream_t s) {
    switch (K) {
        case 1: return stereo_launch_match_k<RIGHT, 1>(a, grid, lds, s);
        case 2: return stereo_launch_match_k<RIGHT, 2>(a, grid, lds, s);
        case 4: return stereo_launch_match_k<RIGHT, 4>(a, grid, lds, s);
        case 8: return stereo_launch_match_k<RIGHT, 8>(a, grid, lds, s);
        default: return stereo_launch_match_k<RIGHT, 16>(a, grid, lds, s);
    }
}

// counts per block (already in p->blk) -> offsets and per-pair counts
static void stereo_launch_scan(pcs_stereo_matcher *p, int64_t n, int64_t nblk, int64_t *d_counts, hipStream_t s) {
    hipLaunchKernelGGL(stereo_scan_kernel, dim3(1), dim3(1024), 0, s, p->blk.as<const int32_t>(), n * nblk, (int)nblk, (int)n, p->off.as<int64_t>(), d_counts);
}

// ---- semi-global matching (ba_stereo_sgm.hpp) -------------------------------------------------------------------------------------------
// S takes 2 H W Dpad bytes per pair (2.6 GB at 2448 x 2048 with 256 disparities), so a batch is walked in chunks of pairs whose S and
// census planes fit the handle's limit.  The default holds six such pairs: the path kernel's parallelism is lines x pairs, and one
// line is one wave.
constexpr int64_t SGM_DEFAULT_WORKSPACE = (int64_t)16 << 30;

struct SgmPlan {
    int rw, rh, K, Dpad;
    int xs0, xs1, ys0, ys1;   // the strict rectangle (ends exclusive; empty: xs1 == xs0 or ys1 == ys0)
    int64_t pair_bytes;       // sgm_pair_bytes: S and the two census planes of one pair
};

static SgmPlan sgm_plan(int W, int H, int min_disp, int D, int census_w, int census_h) {
    SgmPlan t{};
    t.rw = census_w / 2, t.rh = census_h / 2, t.K = sgm_k(D), t.Dpad = sgm_dpad(D);
    const int dmax = min_disp + D - 1;
    t.xs0 = t.rw + std::max(dmax, 0), t.xs1 = std::max(W - t.rw + std::min(min_disp, 0), t.xs0);
    t.ys0 = t.rh, t.ys1 = std::max(H - t.rh, t.ys0);
    t.pair_bytes = sgm_pair_bytes(W, H, t.Dpad);
    return t;
}

// Every argument of pcs_stereo_sgm but the handle: nothing here touches the device.
static int sgm_check(const char *who, int64_t n, int width, int height, const void *d_left, int64_t left_pitch, const void *d_right, int64_t right_pitch, int min_disp, int num_disp,
                     int census_w, int census_h, int p1, int p2, int paths, int uniqueness_ratio, int lr_max_diff, const void *d_valid_left, const void *d_valid_right,
                     const void *d_disp) {
    if (const int rc = stereo_check_shape(who, n, width, height)) return rc;
    if (min_disp < -STEREO_MAX_DISP || min_disp > STEREO_MAX_DISP) return fail(PCS_ERR_ARG, "%s: min_disp %d outside [-%d, %d]", who, min_disp, STEREO_MAX_DISP, STEREO_MAX_DISP);
    if (num_disp < 1 || num_disp > SGM_MAX_DISP) return fail(PCS_ERR_ARG, "%s: num_disp %d outside [1, %d]", who, num_disp, SGM_MAX_DISP);
    if (census_w < 3 || census_w % 2 == 0) return fail(PCS_ERR_ARG, "%s: census_w %d must be odd and >= 3", who, census_w);
    if (census_h < 3 || census_h % 2 == 0) return fail(PCS_ERR_ARG, "%s: census_h %d must be odd and >= 3", who, census_h);
    if ((int64_t)census_w * census_h - 1 > SGM_MAX_BITS)
        return fail(PCS_ERR_ARG, "%s: the census window %d x %d has %lld bits, more than %d", who, census_w, census_h, (long long)census_w * census_h - 1, SGM_MAX_BITS);
    if (p1 < 0 || p1 > p2) return fail(PCS_ERR_ARG, "%s: p1 %d outside [0, p2 = %d]", who, p1, p2);
    if (p2 > SGM_MAX_P) return fail(PCS_ERR_ARG, "%s: p2 %d above %d", who, p2, SGM_MAX_P);
    if (paths != 4 && paths != 8) return fail(PCS_ERR_ARG, "%s: paths %d must be 4 or 8", who, paths);
    if (uniqueness_ratio < 0 || uniqueness_ratio > 100) return fail(PCS_ERR_ARG, "%s: uniqueness_ratio %d outside [0, 100]", who, uniqueness_ratio);
    if (lr_max_diff < -1) return fail(PCS_ERR_ARG, "%s: lr_max_diff %d must be >= -1 (-1: no left-right check)", who, lr_max_diff);
    if (left_pitch < width) return fail(PCS_ERR_ARG, "%s: left_pitch %lld below the row size %d", who, (long long)left_pitch, width);
    if (right_pitch < width) return fail(PCS_ERR_ARG, "%s: right_pitch %lld below the row size %d", who, (long long)right_pitch, width);
    if ((d_valid_left == nullptr) != (d_valid_right == nullptr)) return fail(PCS_ERR_ARG, "%s: d_valid_left and d_valid_right come together", who);
    if (n > 0 && (!d_left || !d_right)) return fail(PCS_ERR_ARG, "%s: d_left and d_right (the images) must be given", who);
    if (n > 0 && !d_disp) return fail(PCS_ERR_ARG, "%s: d_disp must be given", who);
    return PCS_OK;
}

// pairs per chunk under `limit` bytes (0: the default); 0 when not even one pair fits
static int64_t sgm_chunk_pairs(int64_t n, int64_t pair_bytes, int64_t limit) { return std::min(n, (limit > 0 ? limit : SGM_DEFAULT_WORKSPACE) / pair_bytes); }

template <int K>
static void sgm_launch_paths(const SgmArgs &a, int paths, hipStream_t s) {
    static const int dirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};   // (dy, dx)
    const int Ws = a.xs1 - a.xs0, Hs = a.ys1 - a.ys0;
    for (int i = 0; i < paths; ++i) {
        const int dy = dirs[i][0], dx = dirs[i][1], group = dy == 0 ? SGM_HORIZONTAL : dx == 0 ? SGM_VERTICAL : SGM_DIAGONAL;
        const dim3 grid((unsigned)((sgm_line_count(group, Ws, Hs) + SGM_WAVES - 1) / SGM_WAVES), (unsigned)a.nc), block(64 * SGM_WAVES);
        if (group == SGM_HORIZONTAL) hipLaunchKernelGGL((sgm_path_kernel<SGM_HORIZONTAL, K>), grid, block, 0, s, a, dy, dx, (int)(i == 0));
        else if (group == SGM_VERTICAL) hipLaunchKernelGGL((sgm_path_kernel<SGM_VERTICAL, K>), grid, block, 0, s, a, dy, dx, 0);
        else hipLaunchKernelGGL((sgm_path_kernel<SGM_DIAGONAL, K>), grid, block, 0, s, a, dy, dx, 0);
    }
}

extern "C" {
int pcs_stereo_create(pcs_stereo_matcher **out, int device) {
    if (!out) return fail(PCS_ERR_ARG, "pcs_stereo_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_stereo_create", device)) return rc;
    pcs_stereo_matcher *p = new pcs_stereo_matcher();
    hipError_t e = p->core.create(device);
    if (e == hipSuccess) e = p->timer.create();
    if (e != hipSuccess) {
        const int rc = fail(PCS_ERR_HIP, "pcs_stereo_create: %s", hipGetErrorString(e));
        pcs_stereo_destroy(p);
        return rc;
    }
    *out = p;
    return PCS_OK;
}

int pcs_stereo_destroy(pcs_stereo_matcher *p) {
    if (!p) return PCS_OK;
    p->core.destroy({&p->planes, &p->dr, &p->blk, &p->off, &p->qt, &p->sgm}, {&p->timer});
    delete p;
    return PCS_OK;
}

int pcs_stereo_match(pcs_stereo_matcher *p, int64_t n, int width, int height, const uint8_t *d_left, int64_t left_pitch, const uint8_t *d_right, int64_t right_pitch, int min_disp,
                     int num_disp, int block, int prefilter_cap, int texture_threshold, int uniqueness_ratio, int lr_max_diff, const uint8_t *d_valid_left,
                     const uint8_t *d_valid_right, int16_t *d_disp, int32_t *d_cost, uint8_t *d_status, void *stream) {
    const char *who = "pcs_stereo_match";
    if (const int rc = stereo_check_match(who, n, width, height, d_left, left_pitch, d_right, right_pitch, min_disp, num_disp, block, prefilter_cap, texture_threshold,
                                          uniqueness_ratio, lr_max_diff, d_valid_left, d_valid_right, d_disp))
        return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (n == 0) return PCS_OK;
    const StereoTiling t = stereo_tiling(n, width, height, min_disp, num_disp, block, stereo_env_int("PCS_STEREO_TILE_COLUMNS", 1, STEREO_MAX_TW),
                                          stereo_env_int("PCS_STEREO_STRIP_ROWS", 1, 4096));
    const int64_t npix = n * height * width;
    const bool lr = lr_max_diff >= 0;
    return stereo_run(
        p, stream, p->planes.grows(2 * npix) || (lr && p->dr.grows(npix)),
        [&]() -> int {
            if (const int rc = p->planes.grow(2 * npix, 1)) return rc;
            return lr ? p->dr.grow(npix, sizeof(int16_t)) : PCS_OK;
        },
        [&](hipStream_t s) -> int {
            uint8_t *PL = p->planes.as<uint8_t>(), *PR = PL + npix;
            const unsigned gx = (unsigned)((width + 255) / 256);
            hipLaunchKernelGGL(stereo_prefilter_kernel, dim3(gx, (unsigned)height, (unsigned)(2 * n)), dim3(256), 0, s, d_left, d_right, left_pitch, right_pitch, width, height,
                               prefilter_cap, (int)n, PL, PR);
            const int inv = 16 * (min_disp - 1);
            hipLaunchKernelGGL(stereo_fill_kernel, dim3(gx, (unsigned)height, (unsigned)n), dim3(256), 0, s, width, height, t.xs0, t.xs1, t.ys0, t.ys1, inv, d_disp, d_cost, d_status);
            if (t.xs1 <= t.xs0 || t.ys1 <= t.ys0) return PCS_OK;   // no strict pixel: everything is invalid and nothing else is launched
            StereoMatchArgs a{};
            a.PL = PL, a.PR = PR, a.W = width, a.H = height, a.dmin = min_disp, a.D = num_disp, a.r = t.r, a.TW = t.TW, a.SH = t.SH;
            a.y_begin = t.ys0, a.y_end = t.ys1;
            a.dR = p->dr.as<int16_t>(), a.cap = prefilter_cap, a.tex_thr = texture_threshold, a.uniq = uniqueness_ratio, a.lr = lr_max_diff, a.inv = inv;
            a.vL = d_valid_left, a.vR = d_valid_right, a.disp = d_disp, a.cost = d_cost, a.status = d_status;
            const unsigned gy = (unsigned)((t.ys1 - t.ys0 + t.SH - 1) / t.SH);
            if (lr) {
                a.x_begin = t.xr0, a.x_end = t.xr1;
                if (const int rc = stereo_launch_match<true>(t.K, a, dim3((unsigned)((t.xr1 - t.xr0 + t.TW - 1) / t.TW), gy, (unsigned)n), t.lds, s)) return rc;
            }
            a.x_begin = t.xs0, a.x_end = t.xs1;
            return stereo_launch_match<false>(t.K, a, dim3((unsigned)((t.xs1 - t.xs0 + t.TW - 1) / t.TW), gy, (unsigned)n), t.lds, s);
        });
}

int pcs_stereo_set_sgm_workspace(pcs_stereo_matcher *p, int64_t bytes) {
    if (bytes < 0) return fail(PCS_ERR_ARG, "pcs_stereo_set_sgm_workspace: bytes %lld must be >= 0 (0: the default of %lld)", (long long)bytes, (long long)SGM_DEFAULT_WORKSPACE);
    if (!p) return fail(PCS_ERR_ARG, "pcs_stereo_set_sgm_workspace: NULL handle");
    p->sgm_limit = bytes;
    return PCS_OK;
}

int pcs_stereo_sgm(pcs_stereo_matcher *p, int64_t n, int width, int height, const uint8_t *d_left, int64_t left_pitch, const uint8_t *d_right, int64_t right_pitch, int min_disp,
                   int num_disp, int census_w, int census_h, int p1, int p2, int paths, int uniqueness_ratio, int lr_max_diff, const uint8_t *d_valid_left,
                   const uint8_t *d_valid_right, int16_t *d_disp, int32_t *d_cost, uint8_t *d_status, void *stream) {
    const char *who = "pcs_stereo_sgm";
    if (const int rc = sgm_check(who, n, width, height, d_left, left_pitch, d_right, right_pitch, min_disp, num_disp, census_w, census_h, p1, p2, paths, uniqueness_ratio,
                                 lr_max_diff, d_valid_left, d_valid_right, d_disp))
        return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (n == 0) return PCS_OK;
    const SgmPlan t = sgm_plan(width, height, min_disp, num_disp, census_w, census_h);
    const bool empty = t.xs1 <= t.xs0 || t.ys1 <= t.ys0;   // no strict pixel: everything is invalid and only the fill is launched
    const int64_t chunk = empty ? 0 : sgm_chunk_pairs(n, t.pair_bytes, p->sgm_limit);
    if (!empty && chunk < 1)
        return fail(PCS_ERR_ARG, "%s: one pair of this shape needs %lld bytes of workspace, the limit is %lld (pcs_stereo_set_sgm_workspace)", who, (long long)t.pair_bytes,
                    (long long)(p->sgm_limit > 0 ? p->sgm_limit : SGM_DEFAULT_WORKSPACE));
    const int64_t npix = n * height * width, HW = (int64_t)height * width;
    const bool lr = lr_max_diff >= 0;
    const int last_stage = stereo_env_int("PCS_SGM_LAST_STAGE", 1, 4);   // measurements: stop after the census (1), the paths (2), d_R (3)
    return stereo_run(
        p, stream, p->sgm.grows(chunk * t.pair_bytes) || (lr && p->dr.grows(npix)),
        [&]() -> int {
            if (const int rc = p->sgm.grow(chunk * t.pair_bytes, 1)) return rc;
            return lr ? p->dr.grow(npix, sizeof(int16_t)) : PCS_OK;
        },
        [&](hipStream_t s) -> int {
            const unsigned gx = (unsigned)((width + 255) / 256);
            const int inv = 16 * (min_disp - 1);
            hipLaunchKernelGGL(stereo_fill_kernel, dim3(gx, (unsigned)height, (unsigned)n), dim3(256), 0, s, width, height, t.xs0, t.xs1, t.ys0, t.ys1, inv, d_disp, d_cost, d_status);
            if (empty) return PCS_OK;
            const int Ws = t.xs1 - t.xs0, Hs = t.ys1 - t.ys0;
            for (int64_t c0 = 0; c0 < n; c0 += chunk) {
                const int nc = (int)std::min(chunk, n - c0);
                uint16_t *S = p->sgm.as<uint16_t>();
                uint64_t *cen = reinterpret_cast<uint64_t *>(p->sgm.as<unsigned char>() + 2 * sgm_s_offset(nc, 0, 0, width, height, t.Dpad));
                hipLaunchKernelGGL(sgm_census_kernel, dim3(gx, (unsigned)height, (unsigned)(2 * nc)), dim3(256), 0, s, d_left + c0 * height * left_pitch,
                                   d_right + c0 * height * right_pitch, left_pitch, right_pitch, width, height, t.rw, t.rh, nc, cen);
                if (last_stage == 1) continue;
                SgmArgs a{};
                a.cen = cen, a.S = S, a.W = width, a.H = height, a.nc = nc, a.dmin = min_disp, a.D = num_disp, a.Dpad = t.Dpad;
                a.xs0 = t.xs0, a.xs1 = t.xs1, a.ys0 = t.ys0, a.ys1 = t.ys1, a.p1 = p1, a.p2 = p2;
                if (t.K == 1) sgm_launch_paths<1>(a, paths, s);
                else if (t.K == 2) sgm_launch_paths<2>(a, paths, s);
                else sgm_launch_paths<4>(a, paths, s);
                if (last_stage == 2) continue;
                SgmSelectArgs q{};
                q.S = S, q.W = width, q.H = height, q.dmin = min_disp, q.D = num_disp, q.Dpad = t.Dpad, q.xs0 = t.xs0, q.xs1 = t.xs1, q.ys0 = t.ys0, q.ys1 = t.ys1;
                q.pair0 = c0, q.dR = p->dr.as<int16_t>(), q.uniq = uniqueness_ratio, q.lr = lr_max_diff, q.inv = inv;
                q.vL = d_valid_left, q.vR = d_valid_right, q.disp = d_disp, q.cost = d_cost, q.status = d_status;
                if (lr)
                    hipLaunchKernelGGL(sgm_right_kernel, dim3((unsigned)((Ws + num_disp - 1 + SGM_RIGHT_TX - 1) / SGM_RIGHT_TX), (unsigned)Hs, (unsigned)nc), dim3(SGM_RIGHT_TX), 0, s,
                                       q);
                if (last_stage == 3) continue;
                const dim3 grid((unsigned)((Ws + 63) / 64), (unsigned)Hs, (unsigned)nc);
                if (t.K == 1) hipLaunchKernelGGL(sgm_select_kernel<1>, grid, dim3(64), 0, s, q);
                else if (t.K == 2) hipLaunchKernelGGL(sgm_select_kernel<2>, grid, dim3(64), 0, s, q);
                else hipLaunchKernelGGL(sgm_select_kernel<4>, grid, dim3(64), 0, s, q);
            }
            return PCS_OK;
        });
}

// Q and T are HOST arrays; they are uploaded when they differ from what the handle holds.
int pcs_stereo_reproject(pcs_stereo_matcher *p, int64_t n, int width, int height, const int16_t *d_disp, int invalid_disp, const double *Q, int64_t n_Q, double z_lo, double z_hi,
                         const double *T, void *d_points, int dtype, uint8_t *d_mask, int64_t *d_counts, void *stream) {
    const char *who = "pcs_stereo_reproject";
    if (const int rc = stereo_check_reproject(who, n, width, height, d_disp, Q, n_Q, z_lo, z_hi, T, d_points, dtype, d_mask)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (n == 0) return PCS_OK;
    std::vector<double> qt(12 + 16 * (size_t)n_Q, 0.0);
    if (T) std::copy(T, T + 12, qt.begin());
    std::copy(Q, Q + 16 * n_Q, qt.begin() + 12);
    const bool upload = qt != p->h_qt;
    const int64_t nblk = stereo_blocks_per_pair(width, height), NB = n * nblk;
    const bool grows = (upload && p->qt.grows((int64_t)qt.size())) || (d_counts && (p->blk.grows(NB) || p->off.grows(NB + 1)));
    if (upload) {
        HIPCHK(p->core.quiesce());   // a queued reprojection may still read the old matrices
        p->h_qt.clear();
    }
    return stereo_run(
        p, stream, grows,
        [&]() -> int {
            if (upload) {
                if (const int rc = p->qt.grow((int64_t)qt.size(), sizeof(double))) return rc;
                HIPCHK(hipMemcpy(p->qt.p, qt.data(), sizeof(double) * qt.size(), hipMemcpyHostToDevice));
                p->h_qt = qt;
            }
            if (!d_counts) return PCS_OK;
            if (const int rc = p->blk.grow(NB, sizeof(int32_t))) return rc;
            return p->off.grow(NB + 1, sizeof(int64_t));
        },
        [&](hipStream_t s) -> int {
            StereoReprojArgs a{};
            a.disp = d_disp, a.W = width, a.H = height, a.invalid = invalid_disp, a.T = T ? p->qt.as<const double>() : nullptr, a.Q = p->qt.as<const double>() + 12;
            a.q_per_pair = n_Q > 1, a.lo = z_lo, a.hi = z_hi, a.pts = d_points, a.f32 = dtype == PCS_F32, a.mask = d_mask;
            a.blk = d_counts ? p->blk.as<int32_t>() : nullptr, a.nblk = (int)nblk;
            hipLaunchKernelGGL(stereo_reproject_kernel, dim3((unsigned)nblk, (unsigned)n), dim3(STEREO_PIX_PER_BLOCK), 0, s, a);
            if (d_counts) stereo_launch_scan(p, n, nblk, d_counts, s);
            return PCS_OK;
        });
}

int pcs_stereo_compact(pcs_stereo_matcher *p, int64_t n, int width, int height, const void *d_points, int dtype, const uint8_t *d_mask, const uint8_t *d_values,
                       int64_t values_pitch, void *d_out_points, uint8_t *d_out_values, int64_t *d_counts, void *stream) {
    const char *who = "pcs_stereo_compact";
    if (const int rc = stereo_check_compact(who, n, width, height, d_points, dtype, d_mask, d_values, values_pitch, d_out_points, d_out_values, d_counts)) return rc;
    if (!p) return fail(PCS_ERR_ARG, "%s: NULL handle", who);
    if (n == 0) return PCS_OK;
    const int64_t nblk = stereo_blocks_per_pair(width, height), NB = n * nblk;
    return stereo_run(
        p, stream, p->blk.grows(NB) || p->off.grows(NB + 1),
        [&]() -> int {
            if (const int rc = p->blk.grow(NB, sizeof(int32_t))) return rc;
            return p->off.grow(NB + 1, sizeof(int64_t));
        },
        [&](hipStream_t s) -> int {
            const dim3 grid((unsigned)nblk, (unsigned)n);
            hipLaunchKernelGGL(stereo_count_kernel, grid, dim3(STEREO_PIX_PER_BLOCK), 0, s, d_mask, (int64_t)width * height, (int)nblk, p->blk.as<int32_t>());
            stereo_launch_scan(p, n, nblk, d_counts, s);
            StereoScatterArgs a{};
            a.pts = d_points, a.f32 = dtype == PCS_F32, a.mask = d_mask, a.values = d_values, a.values_pitch = values_pitch, a.W = width, a.H = height, a.nblk = (int)nblk;
            a.off = p->off.as<const int64_t>(), a.out_pts = d_out_points, a.out_values = d_out_values;
            hipLaunchKernelGGL(stereo_scatter_kernel, grid, dim3(STEREO_PIX_PER_BLOCK), 0, s, a);
            return PCS_OK;
        });
}

// Device time of the last call of this handle (match, reproject or compact).
int pcs_stereo_last_kernel_ms(pcs_stereo_matcher *p, float *kernel_ms) {
    return timer_ms("pcs_stereo_last_kernel_ms", p ? &p->timer : nullptr, kernel_ms, "nothing has run yet");
}

}  // extern "C"
