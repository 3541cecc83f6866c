// pcs_solver.inc — the handle-free host side of the solver (included by pcs_engine.hip after pcs_common.inc): everything that takes sizes
// or a BlockLayout rather than a handle.  Schur step, SYRK geometry, dense SPD solve, covariance products and the Levenberg-Marquardt trial
// that pcs_engine and pcs_genchain both run: each handle kind fills an LmTrialDesc and hands in its own normal-equations build.

// The blocked layout of J^T J (NormalArgs, ba_normal.hpp): where the parameter string splits into leading part and trailing group.
struct BlockLayout {
    int64_t n_lead, n_trail, n_ent, trail_off;
    int tb, tg;
    int64_t a_len() const { return n_lead * n_lead; }
    int64_t b_len() const { return n_lead * n_trail; }
    int64_t c_len() const { return n_ent * tb * tb; }
    int64_t h_len() const { return a_len() + b_len() + c_len(); }                      // [A | B | C]
    int64_t packed_len(int64_t n_params) const { return h_len() + n_params + 1; }      // [A | B | C | g | cost]
};
// pcs_normal_layout / pcs_genchain_normal_layout
static void layout_out5(const BlockLayout &L, int64_t n_params, int64_t *out5) {
    out5[0] = L.n_lead; out5[1] = L.n_trail; out5[2] = L.tb; out5[3] = L.packed_len(n_params); out5[4] = n_params;
}

// ---- the Schur step -----------------------------------------------------------------------------------------------------------------------
// The buffers of one step by name: filled once from a trial's pcs_lm_buffers (schur_step) and once from the arguments of the piecewise
// entries (schur_prepare_piece / schur_finish_piece).  The preparation reads the first two groups, the completion the second and third.
struct SchurStep {
    double *packed = nullptr;                                   // the current state [A | B | C | g | cost]
    const double *lambda = nullptr; const uint8_t *fixed = nullptr;
    double *V = nullptr, *S = nullptr, *rhs = nullptr, *dvec = nullptr, *gm = nullptr;
    double *linvt = nullptr, *u = nullptr, *delta = nullptr, *ps_out = nullptr;
    const double *w = nullptr, *xlead = nullptr, *ps_in = nullptr;
    int32_t *status = nullptr;                                  // (optional for the completion)
    // optional, for a trial:
    const int32_t *stop = nullptr, *sel = nullptr;              // stop flag; state selector: when *sel != 0 the inputs lie `alt` doubles further on ...
    int64_t alt = 0, out_alt = 0;                               // ... and the vote / the zeroed state `out_alt` doubles further on
    double *fill = nullptr; int64_t fill_n = 0;                 // the one-launch Cholesky's hand-over workspace, set to its fill value on the way
    double *vote = nullptr, *zero = nullptr; int64_t zero_n = 0;   // this rank's vote word behind the trial state; the trial state, zeroed on the way
};
static SchurStep schur_step(const pcs_lm_buffers *b) {   // state 0 current, the trial string into ps[1]
    SchurStep st;
    st.packed = b->packed[0]; st.lambda = b->lambda; st.V = b->V; st.S = b->S; st.rhs = b->rhs; st.dvec = b->dvec; st.gm = b->gm; st.fixed = b->fixed;
    st.linvt = b->linvt; st.u = b->u; st.status = b->status; st.xlead = b->xlead; st.delta = b->delta; st.ps_in = b->ps[0]; st.ps_out = b->ps[1];
    return st;
}
// the step kernels exist for trailing blocks of 6 (a pose) and of 3 (a point)
template <typename K, typename A>
static int launch_tb(int tb, K k6, K k3, dim3 grid, int threads, hipStream_t s, const A &a) {
    hipLaunchKernelGGL(tb == 6 ? k6 : k3, grid, dim3(threads), 0, s, a);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}
static SchurArgs schur_args(const BlockLayout &L, const SchurStep &st) {
    SchurArgs a{};
    a.sel = st.sel; a.alt = st.alt;
    a.fill = reinterpret_cast<uint64_t *>(st.fill); a.fill_n = st.fill ? st.fill_n : 0;
    a.A = st.packed; a.B = a.A + L.a_len(); a.C = a.B + L.b_len(); a.g = a.C + L.c_len();
    a.fixed = st.fixed; a.lambda = st.lambda;
    a.linvt = st.linvt; a.u = st.u; a.V = st.V; a.S = st.S; a.rhs = st.rhs; a.dvec = st.dvec; a.gm = st.gm; a.status = st.status;
    a.n_lead = L.n_lead; a.n_trail = L.n_trail; a.n_ent = L.n_ent; a.trail_off = L.trail_off;
    a.stop = st.stop;
    return a;
}

static int enqueue_schur_prepare(const BlockLayout &L, const SchurStep &st, hipStream_t s) {
    SchurArgs a = schur_args(L, st);
    auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    // trailing blocks and the leading block are independent: one launch (schur_trail_lead_kernel); V needs the trailing factors
    const int64_t nbt = (L.n_lead + 31) / 32, trail_blocks = (L.n_ent + 255) / 256;
    a.trail_blocks = (int32_t)trail_blocks;
    if (trail_blocks + nbt * nbt > 0) {
        const int rc = launch_tb(L.tb, schur_trail_lead_kernel<6>, schur_trail_lead_kernel<3>, dim3((unsigned)(trail_blocks + nbt * nbt)), 256, s, a);
        if (rc) return rc;
    }
    if (L.n_ent > 0 && L.n_lead > 0) return launch_tb(L.tb, schur_v_kernel<6>, schur_v_kernel<3>, blocks(L.n_lead * L.n_ent), 256, s, a);
    return PCS_OK;
}

// The fused forms of the trial's small kernels (csrc/ba_lm_fused.hpp).
static int enqueue_schur_prep_fused(const BlockLayout &L, const SchurStep &st, hipStream_t s) {
    SchurArgs a = schur_args(L, st);
    const int epb = prep_epb(L.tb);
    const int64_t ent_chunks = (L.n_ent + epb - 1) / epb, row_chunks = std::max<int64_t>(1, (L.n_lead + PREP_RPB - 1) / PREP_RPB);
    const int64_t nbt = (L.n_lead + 31) / 32;
    a.ent_chunks = (int32_t)ent_chunks;
    a.trail_blocks = (int32_t)(ent_chunks * row_chunks);
    const int64_t grid = ent_chunks * row_chunks + nbt * nbt;
    if (grid <= 0) return PCS_OK;
    if (grid > INT32_MAX) return fail(PCS_ERR_ARG, "pcs_lm_trial_build: the system is too large for one launch of the Schur preparation");
    return launch_tb(L.tb, schur_prep_kernel<6>, schur_prep_kernel<3>, dim3((unsigned)grid), 256, s, a);
}

static int enqueue_schur_finish(const BlockLayout &L, const SchurStep &st, int n_cu, hipStream_t s) {
    SchurBackArgs a{};
    a.zero = st.zero; a.zero_n = st.zero ? st.zero_n : 0;
    a.sel = st.sel; a.vote = st.vote; a.vote_alt = st.out_alt; a.status = st.status;
    a.linvt = st.linvt; a.u = st.u; a.w = st.w; a.xl = st.xlead; a.fixed = st.fixed; a.delta = st.delta;
    a.ps_in = st.ps_in; a.ps_out = st.ps_out; a.stop = st.stop;
    a.n_lead = L.n_lead; a.n_ent = L.n_ent; a.trail_off = L.trail_off;
    const int64_t n = std::max(L.n_lead, L.n_ent);
    // with a buffer to zero on the way: enough workgroups for that as well (8 doubles per thread and pass, at most four workgroups per CU)
    const int64_t zero_blocks = a.zero ? std::min<int64_t>((a.zero_n / 8 + 255) / 256, (int64_t)n_cu * 4) : 0;
    const dim3 grid((unsigned)std::max<int64_t>((n + 255) / 256, zero_blocks));
    return launch_tb(L.tb, schur_back_kernel<6>, schur_back_kernel<3>, grid, 256, s, a);
}

// what schur_finish_kernel prepares for the build that follows it, beyond the step itself: the hand-fused engines' slabs and point copy
// (a generated chain has its own preparation: all of it empty)
struct FinishSlabs {
    double *cam_slab = nullptr, *pose_slab = nullptr, *points = nullptr;
    int64_t n_cams = 0, n_imgs = 0, n_keys = 0, extr_off = 0, pose_off = 0, point_off = 0;
    bool has_pose = false, copy_points = false;
};
// st.zero = the trial state's packed buffer (zeroed here, the whole of it)
static int enqueue_schur_finish_fused(const BlockLayout &L, int64_t n_params, int n_cu, const FinishSlabs &fs, const SchurStep &st, hipStream_t s) {
    SchurFinishArgs a{};
    a.V = st.V; a.xl = st.xlead; a.n_lead = (int32_t)L.n_lead; a.n_trail = (int32_t)L.n_trail; a.ldv = (int32_t)std::max<int64_t>(1, L.n_trail);
    a.linvt = st.linvt; a.u = st.u; a.fixed = st.fixed; a.delta = st.delta; a.ps_in = st.ps_in; a.ps_out = st.ps_out;
    a.n_ent = L.n_ent; a.trail_off = L.trail_off;
    a.stop = st.stop; a.sel = st.sel;
    a.vote = st.vote; a.vote_alt = st.out_alt; a.status = st.status;
    a.cam_slab = fs.cam_slab; a.pose_slab = fs.pose_slab; a.points = fs.points;
    a.n_cams = (int32_t)fs.n_cams; a.n_imgs = (int32_t)fs.n_imgs; a.n_keys = (int32_t)fs.n_keys;
    a.has_pose = fs.has_pose; a.copy_points = fs.copy_points;
    a.extr_off = fs.extr_off; a.pose_off = fs.pose_off; a.point_off = fs.point_off;
    a.Hm = st.zero; a.n_h = L.h_len(); a.g = a.Hm + a.n_h; a.n_g = n_params; a.cost = a.g + n_params; a.alt_out = st.out_alt;
    const int ecb = finish_ecb(L.tb);
    const int64_t w_blocks = (L.n_ent + ecb - 1) / ecb;
    const bool lead_poses = a.has_pose && fs.pose_off < L.trail_off;
    const int64_t lead_threads = std::max<int64_t>(L.n_lead, fs.n_cams * CAM_STRIDE + (lead_poses ? fs.n_imgs * POSE_STRIDE : 0));
    const int64_t lead_blocks = std::max<int64_t>(1, (lead_threads + 1023) / 1024);
    const int64_t zero_blocks = std::min<int64_t>((a.n_h / 2 + 1023) / 1024 + 1, (int64_t)n_cu * 4);
    a.w_blocks = (int32_t)w_blocks; a.lead_blocks = (int32_t)lead_blocks;
    const int64_t grid = w_blocks + lead_blocks + zero_blocks;
    if (grid > INT32_MAX) return fail(PCS_ERR_ARG, "pcs_lm_trial_build: the system is too large for one launch of the step's completion");
    return launch_tb(L.tb, schur_finish_kernel<6>, schur_finish_kernel<3>, dim3((unsigned)grid), 1024, s, a);
}

// The pieces of a trial as calls of their own, for a loop the HOST steers (a sharded solve whose collective goes through the host, and
// tests): pcs_schur_prepare / pcs_schur_finish / pcs_lm_decide and their pcs_genchain_* twins check their handle, resolve the stream and
// come here with its device and layout.  The caller runs pcs_schur_syrk, pcs_dense_spd_solve and pcs_schur_vtx (sizes, not handles) in between.
static int schur_prepare_piece(const char *who, int device, const BlockLayout &L, hipStream_t s, double *d_packed, const uint8_t *d_fixed, const double *d_lambda,
                               double *d_linvt, double *d_u, double *d_V, double *d_S, double *d_rhs, double *d_dvec, double *d_gm, int32_t *d_status) {
    if (!d_packed || !d_fixed || !d_lambda || !d_linvt || !d_u || !d_V || !d_S || !d_rhs || !d_dvec || !d_gm || !d_status) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    HIPCHK(hipSetDevice(device));
    SchurStep st;
    st.packed = d_packed; st.fixed = d_fixed; st.lambda = d_lambda; st.linvt = d_linvt; st.u = d_u; st.V = d_V; st.S = d_S; st.rhs = d_rhs;
    st.dvec = d_dvec; st.gm = d_gm; st.status = d_status;
    return enqueue_schur_prepare(L, st, s);
}
static int schur_finish_piece(const char *who, int device, const BlockLayout &L, hipStream_t s, const double *d_linvt, const double *d_u, const double *d_w,
                              const double *d_xlead, const uint8_t *d_fixed, double *d_delta, const double *d_ps_in, double *d_ps_out) {
    if (!d_linvt || !d_u || !d_w || !d_xlead || !d_fixed || !d_delta || ((d_ps_in == nullptr) != (d_ps_out == nullptr))) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    HIPCHK(hipSetDevice(device));
    SchurStep st;
    st.linvt = const_cast<double *>(d_linvt); st.u = const_cast<double *>(d_u);   // (read only by the completion)
    st.w = d_w; st.xlead = d_xlead; st.fixed = d_fixed; st.delta = d_delta; st.ps_in = d_ps_in; st.ps_out = d_ps_out;
    return enqueue_schur_finish(L, st, 256, s);
}
static int lm_decide_piece(const char *who, int device, int64_t n_params, hipStream_t s, const double *d_cost_old, const double *d_cost_new, const double *d_dvec,
                           const double *d_gm, const double *d_delta, const double *d_ps, const uint8_t *d_fixed, int32_t *d_status, double *d_lambda, double *d_stats,
                           const double *d_alpha = nullptr, uint8_t *d_pin = nullptr) {
    if (!d_cost_old || !d_cost_new || !d_dvec || !d_gm || !d_delta || !d_ps || !d_fixed || !d_status || !d_lambda || !d_stats) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    HIPCHK(hipSetDevice(device));
    LmDecideArgs a{};
    a.tail[0] = d_cost_old; a.tail[1] = d_cost_new; a.ps2[0] = a.ps2[1] = d_ps;
    a.dvec = d_dvec; a.gm = d_gm; a.delta = d_delta; a.fixed = d_fixed; a.status = d_status; a.lambda = d_lambda; a.stats = d_stats; a.n_params = n_params;
    a.alpha = d_alpha;   // pcs_lm_decide_bounded; NULL: pcs_lm_decide
    a.pin = d_pin;
    hipLaunchKernelGGL(lm_decide_kernel, dim3(1), dim3(1024), 0, s, a);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}

// launch geometry of S -= V V' (csrc/ba_schur.hpp): tile width, tiles of the lower triangle, K split.  `ordered` = the partial sums of a
// split go through a workspace and are subtracted in order (deterministic mode) instead of meeting in atomics.
struct SyrkGeometry { bool big; int64_t tw, tiles, ksplit, kchunk; };
static SyrkGeometry syrk_geometry(int64_t n_lead, int64_t n_trail, bool ordered) {
    // 64 x 64 tiles once 32 x 32 ones alone would fill the chip twice over (their operand traffic, not the matrix cores, is the bound then:
    // rig-32-self 175 us -> ~100 us); PCS_SYRK_TILE=32 / 64 forces one form (A/B)
    static const int forced = getenv("PCS_SYRK_TILE") ? atoi(getenv("PCS_SYRK_TILE")) : 0;
    const int64_t nb32 = (n_lead + 31) / 32;
    SyrkGeometry g{};
    g.big = forced == 64 || (forced != 32 && nb32 * (nb32 + 1) / 2 >= 1024);
    g.tw = g.big ? 64 : 32;
    const int64_t nb = (n_lead + g.tw - 1) / g.tw;
    g.tiles = nb * (nb + 1) / 2;
    // split K until ~512 workgroups exist (rig-32: 120 tiles x 5; the 2e4-point free chain: 21 tiles x 25 of 60 000 columns)
    int64_t ksplit = std::min<int64_t>((512 + g.tiles - 1) / g.tiles, (n_trail + 127) / 128);
    ksplit = std::max<int64_t>(1, ksplit);
    int64_t kchunk = ((n_trail + ksplit - 1) / ksplit + 63) / 64 * 64;
    ksplit = (n_trail + kchunk - 1) / kchunk;
    if (g.big) {
        // 64 x 64 tiles run two workgroups per CU: split K so that the workgroups fill whole rounds of the resident ones — the cost of a
        // split = rounds x (columns per workgroup + ~64 columns' worth of ramp and atomics); rig-32-self: 378 tiles x 4 = 2.95 rounds.
        // Ordered mode: every split also writes and re-reads a 32 KB partial tile (rig-32-self: 50 MB per solve for four splits) —
        // priced as 48 more columns per split.  (Priced at 192 the model left rig-32-self unsplit: 378 workgroups of 1 458 columns on
        // 512 slots took 172.7 us against 133.4 us for the four-way split with atomics, profiles/r05/lm_trace_rig32_self_form11.log.)
        int dev = 0;
        const int cus = hipGetDevice(&dev) == hipSuccess && device_cu_count(dev) > 0 ? device_cu_count(dev) : 256;
        const int64_t slots = 2 * (int64_t)cus;
        int64_t best = INT64_MAX;
        for (int64_t ks = 1; ks <= std::max<int64_t>(1, n_trail / 128); ++ks) {
            const int64_t kc = ((n_trail + ks - 1) / ks + 63) / 64 * 64, real = (n_trail + kc - 1) / kc;
            const int64_t cost = (g.tiles * real + slots - 1) / slots * (kc + 64 + ((ordered && real > 1) ? 48 : 0));
            if (cost < best) { best = cost; ksplit = real; kchunk = kc; }
        }
    }
    g.ksplit = ksplit; g.kchunk = kchunk;
    return g;
}
// doubles of the ordered mode's workspace (0: the product is not split, nothing is needed)
static int64_t syrk_work_doubles(int64_t n_lead, int64_t n_trail) {
    const SyrkGeometry g = syrk_geometry(n_lead, n_trail, true);
    return g.ksplit > 1 ? g.ksplit * (g.tiles * g.tw * g.tw + n_lead) : 0;
}

// the operands of S -= V V' (and rhs -= V u when u is given); ws = the ordered mode's workspace (NULL: atomics)
struct SyrkOperands { const double *V; int64_t ldv; double *S; int64_t lds; const double *u; double *rhs; double *ws = nullptr; int64_t ws_doubles = 0; };
static int enqueue_schur_syrk(int64_t n_lead, int64_t n_trail, const SyrkOperands &m, hipStream_t s, const int32_t *d_stop) {
    const bool ordered = m.ws != nullptr;
    const SyrkGeometry g = syrk_geometry(n_lead, n_trail, ordered);
    if (ordered && g.ksplit > 1 && m.ws_doubles < g.ksplit * (g.tiles * g.tw * g.tw + n_lead))
        return fail(PCS_ERR_ARG, "pcs_schur_syrk: the ordered mode needs a workspace of %lld doubles (pcs_schur_syrk_work_len), got %lld",
                    (long long)(g.ksplit * (g.tiles * g.tw * g.tw + n_lead)), (long long)m.ws_doubles);
    SchurSyrkArgs a{m.V, m.S, m.u, m.rhs, (int32_t)n_lead, (int32_t)n_trail, (int32_t)m.ldv, (int32_t)m.lds, (int32_t)g.ksplit, (int32_t)g.kchunk, d_stop};
    a.ws = (ordered && g.ksplit > 1) ? m.ws : nullptr;
    a.ws_rhs = a.ws ? m.ws + g.ksplit * g.tiles * g.tw * g.tw : nullptr;
    a.tiles = (int32_t)g.tiles;
    if (g.big) hipLaunchKernelGGL(schur_syrk64_kernel, dim3((unsigned)(g.tiles * g.ksplit)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(schur_syrk_kernel, dim3((unsigned)(g.tiles * g.ksplit)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    if (a.ws) {
        if (g.big) hipLaunchKernelGGL(schur_syrk_reduce_kernel<64>, dim3((unsigned)(g.tiles * 16)), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(schur_syrk_reduce_kernel<32>, dim3((unsigned)(g.tiles * 4)), dim3(256), 0, s, a);
        HIPCHK(hipGetLastError());
    }
    return PCS_OK;
}

// does a solve of size n with this algorithm request take the ONE persistent launch (csrc/ba_chol_persist.hpp)?  Wherever its tiles fit
// the chip's LDS: n <= 1 984 on 256 CUs.  (Round 5 also tried ONE workgroup with the whole matrix in its LDS for n <= 160 — nothing to hand
// over —: 110 us at n = 120 against the persistent kernel's 47: fourteen workgroups load, update and factor their tiles side by side, one
// workgroup does it all in sequence.  Dropped.)
static bool dense_spd_is_one_launch(int device, int64_t n, int algorithm) {
    return n > 0 && cp_fits(n, device_cu_count(device)) && (algorithm == PCS_SPD_ONE_LAUNCH || algorithm == PCS_SPD_AUTO);
}

struct SpdSystem { double *S; int64_t ld; const double *rhs; double *x, *work; int32_t *status; };
struct SpdOptions { int algorithm = PCS_SPD_AUTO; const int32_t *stop = nullptr; bool prefilled = false; int64_t timeout_us = 250000; };   // prefilled: the hand-over workspace of the one-launch form is at its fill value
static int enqueue_dense_spd(int device, int64_t n, const SpdSystem &m, const SpdOptions &o, void *stream) {
    constexpr int NB = 32;
    if (n <= 0 || n > (1 << 15) || m.ld < n || !m.S || !m.rhs || !m.x || !m.work || !m.status) return fail(PCS_ERR_ARG, "pcs_dense_spd_solve: bad arguments");
    if (o.algorithm != PCS_SPD_AUTO && o.algorithm != PCS_SPD_LAUNCHES && o.algorithm != PCS_SPD_ONE_LAUNCH) return fail(PCS_ERR_ARG, "pcs_dense_spd_solve: unknown algorithm %d", o.algorithm);
    if (device < 0 || device >= pcs_device_count()) return fail(PCS_ERR_NODEVICE, "pcs_dense_spd_solve: device %d not available", device);
    HIPCHK(hipSetDevice(device));
    if (o.algorithm == PCS_SPD_ONE_LAUNCH && !cp_fits(n, device_cu_count(device)))
        return fail(PCS_ERR_ARG, "pcs_dense_spd_solve: n = %lld does not fit the one-launch form on %d compute units", (long long)n, device_cu_count(device));
    if (dense_spd_is_one_launch(device, n, o.algorithm)) {
        HIPCHK(cp_launch(n, m.S, m.ld, m.rhs, m.x, m.work, m.status, device_cu_count(device), (hipStream_t)stream, 1.0e-6 * (double)o.timeout_us, nullptr, o.stop, o.prefilled));
        return PCS_OK;
    }
    hipStream_t s = (hipStream_t)stream;   // NULL = the default stream
    const int nblk = (int)((n + NB - 1) / NB);
    double *d_ldiag = m.work + (int64_t)nblk * NB * NB;
    double *d_y = d_ldiag + (int64_t)nblk * NB * NB;
    CholArgs a{m.S, m.work, d_ldiag, m.status, (int32_t)n, (int32_t)m.ld, 0, m.rhs, d_y, o.stop};
    a.k = 0;
    hipLaunchKernelGGL(chol_panel_kernel<NB>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    for (int k = 0; k + 1 < nblk; ++k) {   // trailing update with column k + panel step of column k + 1, one launch
        a.k = k;
        const int mm = nblk - k - 1;
        hipLaunchKernelGGL(chol_step_kernel<NB>, dim3((unsigned)(mm * (mm + 1) / 2)), dim3(256), 0, s, a);
    }
    HIPCHK(hipGetLastError());
    // backward sweep L' x = y: pieces of at most 16 blocks in one workgroup each, lower-right first; between two pieces a GEMV over
    // many workgroups takes the solved rows out of the rest of y (csrc/ba_dense_chol.hpp)
    struct Rec {
        static void run(hipStream_t s, const CholSolveArgs &base, int kb0, int kb1) {
            constexpr int NBk = 32;
            if (kb1 - kb0 <= 16) {
                CholSolveArgs b = base;
                b.kb0 = kb0; b.kb1 = kb1;
                const size_t lds = sizeof(double) * ((size_t)(kb1 - kb0) * NBk + NBk);
                hipLaunchKernelGGL(chol_solve_kernel<NBk>, dim3(1), dim3(512), lds, s, b);
                return;
            }
            const int mid = kb0 + (kb1 - kb0 + 1) / 2;
            run(s, base, mid, kb1);
            const int r0 = mid * NBk, r1 = std::min<int>(kb1 * NBk, base.n), c0 = kb0 * NBk, c1 = mid * NBk;
            hipLaunchKernelGGL(chol_gemv_t_kernel, dim3((unsigned)((c1 - c0 + 63) / 64)), dim3(1024), 0, s, (const double *)base.L, (int)base.ld, (const double *)base.x, base.y,
                               r0, r1, c0, c1, base.stop);
            run(s, base, kb0, mid);
        }
    };
    CholSolveArgs b{m.S, m.work, d_ldiag, d_y, m.x, (int32_t)n, (int32_t)m.ld, 0, nblk, o.stop};
    Rec::run(s, b, 0, nblk);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}

// ---- the Levenberg-Marquardt trial -------------------------------------------------------------------------------------------------------
// One whole Levenberg-Marquardt trial in two halves (round 5; pcs_lm_trial = both): BUILD = the damped Schur step from the current state at
// *lambda (+ the trial parameter string) and the normal equations at the trial string into the other state's packed buffer; FINISH = the
// decision INCLUDING the loop's termination rules, the state flip of an accepted trial and the read-back of the twelve numbers the host
// follows the loop with.  A sharded loop puts its all-reduce of the trial state between the two, on the same stream.  Every kernel starts
// with PCS_STOP_GUARD on flags[0], so the host may queue trial t + 1 before it has read the verdict of trial t.
static int lm_check(const void *h, const pcs_lm_buffers *b, const char *who) {
    if (!h || !b || !b->packed[0] || !b->packed[1] || !b->ps[0] || !b->ps[1] || !b->flags || !b->fixed || !b->lambda || !b->linvt || !b->u || !b->V || !b->S || !b->rhs ||
        !b->dvec || !b->gm || !b->status || !b->xlead || !b->w || !b->spd_work || !b->delta || !b->ctrl || !b->stats)
        return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (reinterpret_cast<uintptr_t>(b->packed[0]) % 16 || reinterpret_cast<uintptr_t>(b->packed[1]) % 16) return fail(PCS_ERR_ARG, "%s: the packed buffers must be 16-byte aligned", who);
    if (b->mode & ~(PCS_LM_FIXED_TRIAL_BUFFER | PCS_LM_VOTES)) return fail(PCS_ERR_ARG, "%s: unknown mode bits", who);
    return PCS_OK;
}

// What the BUILD half needs to know about the handle it runs for; pcs_lm_trial_build and pcs_genchain_lm_trial_build fill one each.
struct LmTrialDesc {
    const char *who = "";             // the exported entry point, for error texts
    int device = 0, n_cu = 256; int64_t n_params = 0;
    BlockLayout L{};
    bool deterministic = false;       // S -= V V' through the ordered workspace (pcs_lm_buffers.syrk_work)
    int64_t spd_timeout_us = 250000;
    bool fused = false;               // the two launches in front of the matrix products as one, the three behind the dense solve as one (csrc/ba_lm_fused.hpp).  Both kinds need n_ent > 0 and n_lead > 0 (trailing entities with leading rows to ride on); the engine also its "fused_trial" option and a table (n > 0: the build's prologue is theirs to replace)
    bool selector = false;            // flags[2] selects the current one of two states (the engine); false: state 0 is always current (generated chains: sel = NULL, alt = 0)
    bool finish_zeroes = false;       // the NON-fused completion zeroes packed[1] on the way (generated chains: their contraction sums into it); false: the build's own prologue does (the engine)
    FinishSlabs slabs;                // what the fused completion prepares for the build (the engine's slabs; empty for a generated chain)
    const BoundStore *bounds = nullptr;   // the handle's box bounds (csrc/ba_bounds.hpp).  Active: the caller leaves `fused` off — the fused completion prepares the engine's slabs at the trial string in the launch that writes it, and a truncation behind it would leave them stale
    bool empty_zero_state = false;    // the table is empty AND that means a zeroed trial state for a sharded loop's all-reduce (the engine: n == 0; needs PCS_LM_FIXED_TRIAL_BUFFER); a generated chain leaves it false: its build refuses an empty table
};

// The handle's box bounds (BoundStore, csrc/ba_bounds.hpp) around a Schur step.  `ps`, `g`: the strings and the gradients of the two states, the
// current one named by *sel (NULL: state 0); one launch of one workgroup each, behind the stop word like every kernel of a trial.
struct BoundsTarget { double *ps[2]; const double *g[2]; const int32_t *sel = nullptr, *stop = nullptr; };
static BoundsArgs bounds_args(const BoundStore &bs, int64_t n_params, const BoundsTarget &t) {
    BoundsArgs a{};
    a.lo = bs.lo(); a.hi = bs.hi(); a.pin = bs.pin(); a.n_params = n_params;
    a.ps[0] = t.ps[0]; a.ps[1] = t.ps[1]; a.g[0] = t.g[0]; a.g[1] = t.g[1]; a.sel = t.sel; a.stop = t.stop;
    return a;
}
// fixed_eff <- fixed or "on a bound with the gradient pointing out" at the current state; *n_active <- how many entries the bounds added
static int enqueue_bounds_active(const BoundStore &bs, int64_t n_params, const BoundsTarget &t, const uint8_t *fixed, uint8_t *fixed_eff, int32_t *n_active, hipStream_t s) {
    BoundsArgs a = bounds_args(bs, n_params, t);
    a.fixed = fixed; a.fixed_eff = fixed_eff; a.n_active = n_active;
    hipLaunchKernelGGL(bounds_active_kernel, dim3(1), dim3(BOUNDS_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}
// the step `delta` from the current string cut at the first bound: delta, the trial string and *alpha
static int enqueue_bounds_truncate(const BoundStore &bs, int64_t n_params, const BoundsTarget &t, double *delta, double *alpha, hipStream_t s) {
    BoundsArgs a = bounds_args(bs, n_params, t);
    a.delta = delta; a.alpha = alpha;
    hipLaunchKernelGGL(bounds_truncate_kernel, dim3(1), dim3(BOUNDS_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}
// pcs_bounds_active_device / pcs_bounds_truncate_device and their pcs_genchain_* twins
static int bounds_active_piece(const char *who, int device, const BoundStore &bs, const BlockLayout &L, int64_t n_params, const double *d_ps, const double *d_packed,
                               const uint8_t *d_fixed, uint8_t *d_fixed_eff, hipStream_t s) {
    if (!d_ps || !d_packed || !d_fixed || !d_fixed_eff) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (!bs.active()) return fail(PCS_ERR_STATE, "%s: no bounds set", who);
    HIPCHK(hipSetDevice(device));
    double *ps = const_cast<double *>(d_ps);   // (read only by this kernel)
    const BoundsTarget t{{ps, ps}, {d_packed + L.h_len(), d_packed + L.h_len()}};
    return enqueue_bounds_active(bs, n_params, t, d_fixed, d_fixed_eff, bs.n_active(), s);
}
// the same two for a caller that keeps TWO states and a selector word, as pcs_lm_trial_build does (pcs_bounds_*_sel_device)
static int bounds_active_sel_piece(const char *who, int device, const BoundStore &bs, const BlockLayout &L, int64_t n_params, const double *d_ps0, const double *d_ps1,
                                   const double *d_packed0, const double *d_packed1, const uint8_t *d_fixed, uint8_t *d_fixed_eff, const int32_t *d_sel, hipStream_t s) {
    if (!d_ps0 || !d_ps1 || !d_packed0 || !d_packed1 || !d_fixed || !d_fixed_eff || !d_sel) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (!bs.active()) return fail(PCS_ERR_STATE, "%s: no bounds set", who);
    HIPCHK(hipSetDevice(device));
    BoundsTarget t{{const_cast<double *>(d_ps0), const_cast<double *>(d_ps1)}, {d_packed0 + L.h_len(), d_packed1 + L.h_len()}};   // (read only by this kernel)
    t.sel = d_sel;
    return enqueue_bounds_active(bs, n_params, t, d_fixed, d_fixed_eff, bs.n_active(), s);
}
static int bounds_truncate_sel_piece(const char *who, int device, const BoundStore &bs, int64_t n_params, double *d_ps0, double *d_ps1, double *d_delta, double *d_alpha,
                                     const int32_t *d_sel, hipStream_t s) {
    if (!d_ps0 || !d_ps1 || d_ps0 == d_ps1 || !d_delta || !d_alpha || !d_sel) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (!bs.active()) return fail(PCS_ERR_STATE, "%s: no bounds set", who);
    HIPCHK(hipSetDevice(device));
    BoundsTarget t{{d_ps0, d_ps1}, {nullptr, nullptr}};
    t.sel = d_sel;
    return enqueue_bounds_truncate(bs, n_params, t, d_delta, d_alpha, s);
}
static int bounds_truncate_piece(const char *who, int device, const BoundStore &bs, int64_t n_params, const double *d_ps_in, double *d_delta, double *d_ps_out,
                                 double *d_alpha, hipStream_t s) {
    if (!d_ps_in || !d_delta || !d_ps_out || !d_alpha || d_ps_in == d_ps_out) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (!bs.active()) return fail(PCS_ERR_STATE, "%s: no bounds set", who);
    HIPCHK(hipSetDevice(device));
    const BoundsTarget t{{const_cast<double *>(d_ps_in), d_ps_out}, {nullptr, nullptr}};
    return enqueue_bounds_truncate(bs, n_params, t, d_delta, d_alpha, s);
}

// build_trial(stream, fused) = the handle's own normal equations at ps[1] into packed[1]; fused: the completion has done its prologue's work.
// (The guards on n_lead > 0 never bite: every layout either handle kind makes has leading columns.)
template <typename BuildTrial>
static int enqueue_lm_trial_build(const LmTrialDesc &d, const pcs_lm_buffers *b, hipStream_t s, BuildTrial &&build_trial) {
    const BlockLayout &L = d.L;
    const int64_t n_packed = L.packed_len(d.n_params);
    const int64_t alt_pk = d.selector ? b->packed[1] - b->packed[0] : 0;   // doubles from state 0 to state 1
    SchurStep st = schur_step(b);
    st.stop = b->flags;
    if (d.selector) { st.sel = b->flags + 2; st.alt = alt_pk; }
    st.out_alt = -alt_pk;
    // box bounds: the active set of the CURRENT state (for a sharded loop the all-reduced one with the prior added: the same bits on every
    // rank) takes the place of the caller's mask in the step; nothing is queued without bounds
    const bool bounded = d.bounds && d.bounds->active();
    if (bounded && d.fused) return fail(PCS_ERR_STATE, "%s: a bounded trial takes the non-fused sequence", d.who);
    const BoundsTarget bt{{b->ps[0], b->ps[1]}, {b->packed[0] + L.h_len(), b->packed[1] + L.h_len()}, st.sel, st.stop};
    if (bounded) {
        if (const int brc = enqueue_bounds_active(*d.bounds, d.n_params, bt, b->fixed, d.bounds->fixed_eff(), d.bounds->n_active(), s)) return brc;
        st.fixed = d.bounds->fixed_eff();
    }
    // the one-launch Cholesky wants its hand-over workspace at the fill value: the preparation sets it on the way (one launch fewer)
    const bool prefill = L.n_lead > 0 && dense_spd_is_one_launch(d.device, L.n_lead, b->spd_algorithm);
    if (prefill) { st.fill = b->spd_work; st.fill_n = cp_work_doubles((L.n_lead + 31) / 32); }
    int rc = d.fused ? enqueue_schur_prep_fused(L, st, s) : enqueue_schur_prepare(L, st, s);
    if (rc) return rc;
    const int64_t ldv = std::max<int64_t>(1, L.n_trail);
    if (L.n_trail > 0 && L.n_lead > 0) {
        if (d.deterministic && !b->syrk_work && syrk_work_doubles(L.n_lead, L.n_trail) > 0)
            return fail(PCS_ERR_ARG, "%s: deterministic mode needs pcs_lm_buffers.syrk_work (pcs_schur_syrk_work_len doubles)", d.who);
        rc = enqueue_schur_syrk(L.n_lead, L.n_trail, SyrkOperands{b->V, ldv, b->S, L.n_lead, b->u, b->rhs, d.deterministic ? b->syrk_work : nullptr, b->syrk_work_len}, s, st.stop);
        if (rc) return rc;
    }
    st.w = b->u;
    if (L.n_lead > 0) {
        rc = enqueue_dense_spd(d.device, L.n_lead, SpdSystem{b->S, L.n_lead, b->rhs, b->xlead, b->spd_work, b->status},
                               SpdOptions{b->spd_algorithm, st.stop, prefill, d.spd_timeout_us}, s);
        if (rc) return rc;
        if (L.n_trail > 0 && !d.fused) {
            launch_schur_vtx(b->V, b->xlead, b->w, (int)L.n_lead, (int)L.n_trail, (int)ldv, st.stop, s);
            HIPCHK(hipGetLastError());
            st.w = b->w;
        }
    }
    // this rank's vote behind the TRIAL state's packed buffer (ps[1] / packed[1] while state 0 is current)
    st.vote = (b->mode & PCS_LM_VOTES) ? b->packed[1] + n_packed : nullptr;
    if (d.fused || d.finish_zeroes) { st.zero = b->packed[1]; st.zero_n = n_packed; }
    // fused: w = V' x_l, the back substitution, the step, the trial string, the vote, the engine's slabs at the trial string and the zeroed
    // trial state in ONE launch; else the step, the trial string and the vote
    rc = d.fused ? enqueue_schur_finish_fused(L, d.n_params, d.n_cu, d.slabs, st, s) : enqueue_schur_finish(L, st, d.n_cu, s);
    if (rc) return rc;
    if (bounded) {   // the step stops at the first bound it meets, in front of the build (whose own prologue prepares the slabs from the trial string)
        rc = enqueue_bounds_truncate(*d.bounds, d.n_params, bt, b->delta, d.bounds->alpha(), s);
        if (rc) return rc;
    }
    if (d.empty_zero_state) {
        // a rank whose observation shard is empty (ceil(N / world) rows per rank can leave the last ranks without any) contributes zeros
        // to the all-reduce of the trial state; the vote word behind it stays
        if (!(b->mode & PCS_LM_FIXED_TRIAL_BUFFER)) return fail(PCS_ERR_STATE, "no detections set");
        HIPCHK(hipMemsetAsync(b->packed[1], 0, sizeof(double) * (size_t)n_packed, s));
        return PCS_OK;
    }
    return build_trial(s, d.fused);
}

// The handle's prior (PriorStore, csrc/ba_prior.hpp) onto a packed state of layout L.  One state: packed / ps with sel = NULL.  A trial's
// finish half: both states and both strings with the selector, the prior goes to the TRIAL ones exactly as lm_decide_kernel reads them; behind
// the stop word like every kernel of a trial.  No prior: nothing is queued.
struct PriorTarget { double *packed[2]; const double *ps[2]; const int32_t *sel = nullptr, *stop = nullptr; };
static int enqueue_prior_add(const PriorStore &pr, const BlockLayout &L, int64_t n_params, const PriorTarget &t, hipStream_t s) {
    if (!pr.active()) return PCS_OK;
    PriorArgs a{};
    a.idx = pr.idx(); a.mean = pr.mean(); a.w = pr.w(); a.n = pr.n;
    a.packed[0] = t.packed[0]; a.packed[1] = t.packed[1]; a.ps[0] = t.ps[0]; a.ps[1] = t.ps[1]; a.sel = t.sel; a.stop = t.stop;
    a.n_lead = L.n_lead; a.trail_off = L.trail_off; a.c_off = L.a_len() + L.b_len(); a.g_off = L.h_len(); a.n_params = n_params; a.tb = L.tb;
    const int64_t wgs = pr.workgroups();
    if (wgs > INT32_MAX) return fail(PCS_ERR_ARG, "the parameter prior is too long for one launch");
    a.partial = wgs > 1 ? pr.partial.as<double>() : nullptr;
    a.n_partial = (int32_t)wgs;
    hipLaunchKernelGGL(prior_add_kernel, dim3((unsigned)wgs), dim3(PRIOR_THREADS), 0, s, a);
    if (wgs > 1) hipLaunchKernelGGL(prior_cost_kernel, dim3(1), dim3(PRIOR_THREADS), 0, s, a);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}
// pcs_prior_add_device / pcs_genchain_prior_add_device
static int prior_add_piece(const char *who, int device, const PriorStore &pr, const BlockLayout &L, int64_t n_params, const double *d_param_str, double *d_packed, hipStream_t s) {
    if (!d_param_str || !d_packed) return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (!pr.active()) return PCS_OK;
    HIPCHK(hipSetDevice(device));
    PriorTarget t{{d_packed, d_packed}, {d_param_str, d_param_str}};
    return enqueue_prior_add(pr, L, n_params, t, s);
}

// The second half of a trial for a state of layout L ([blocks | g | cost]; pcs_engine and pcs_genchain alike).
static int enqueue_lm_finish(int n_cu, int64_t n_params, const BlockLayout &L, const PriorStore &prior, const BoundStore &bounds, const pcs_lm_buffers *b, hipStream_t s) {
    const int64_t n_packed = L.packed_len(n_params);
    const bool fixed_buffer = (b->mode & PCS_LM_FIXED_TRIAL_BUFFER) != 0;
    if (prior.active()) {   // the prior at the trial string onto the trial state (behind a sharded loop's all-reduce), in front of the decision
        PriorTarget t{{b->packed[0], b->packed[1]}, {b->ps[0], b->ps[1]}, b->flags + 2, b->flags};
        if (const int rc = enqueue_prior_add(prior, L, n_params, t, s)) return rc;
    }
    LmDecideArgs a{};
    a.tail[0] = b->packed[0] + n_packed - 1; a.tail[1] = b->packed[1] + n_packed - 1;
    a.ps2[0] = b->ps[0]; a.ps2[1] = b->ps[1];
    a.sel = b->flags + 2;
    a.dvec = b->dvec; a.gm = b->gm; a.delta = b->delta; a.fixed = b->fixed; a.status = b->status; a.lambda = b->lambda; a.stats = b->stats;
    a.n_params = n_params;
    if (bounds.active()) {   // the decision on the truncated step: the effective mask, alpha, and the trial's record for the host
        a.fixed = bounds.fixed_eff(); a.alpha = bounds.alpha(); a.n_active = bounds.n_active();
        a.bound_log = bounds.log(); a.bound_log_trials = BOUNDS_LOG_TRIALS; a.n_truncated = bounds.n_truncated(); a.pin = bounds.pin();
    }
    a.ctrl = b->ctrl; a.stop_flag = b->flags; a.accept_flag = b->flags + 1;
    a.use_votes = (b->mode & PCS_LM_VOTES) ? 1 : 0;
    a.keep_sel = fixed_buffer ? 1 : 0;
    if (b->result_host && b->free_idx && b->n_free > 0) {   // the final state straight into the host's mapped buffer when this trial ends the loop
        double *result_mapped = nullptr;
        if (hipHostGetDevicePointer(reinterpret_cast<void **>(&result_mapped), b->result_host, 0) == hipSuccess && result_mapped) {
            a.free_idx = b->free_idx; a.n_free = b->n_free; a.result = result_mapped;
        } else {
            (void)hipGetLastError();
        }
    }
    // the read-back: lm_decide_kernel writes the twelve numbers straight into the page-locked buffer when the device can address it (no
    // copy launch); a buffer that is not mapped gets an asynchronous copy
    double *stats_mapped = nullptr;
    if (b->stats_host && hipHostGetDevicePointer(reinterpret_cast<void **>(&stats_mapped), b->stats_host, 0) != hipSuccess) {
        (void)hipGetLastError();
        stats_mapped = nullptr;
    }
    a.stats_host = stats_mapped;
    hipLaunchKernelGGL(lm_decide_kernel, dim3(1), dim3(1024), 0, s, a);
    HIPCHK(hipGetLastError());
    if (b->stats_host && !stats_mapped) HIPCHK(hipMemcpyAsync(b->stats_host, b->stats, sizeof(double) * LM_STATS, hipMemcpyDeviceToHost, s));
    if (fixed_buffer) {   // the trial state sits in a fixed buffer (the one a sharded loop's all-reduce was queued on) — an accepted one is copied over the current state
        const int copy_blocks = (int)std::min<int64_t>((n_packed / 2 + 255) / 256 + 1, (int64_t)n_cu * 8);
        hipLaunchKernelGGL(lm_accept_kernel, dim3((unsigned)copy_blocks), dim3(256), 0, s, (const int32_t *)(b->flags + 1), (const double *)b->packed[1], b->packed[0], n_packed,
                           (const double *)b->ps[1], b->ps[0], n_params);
        HIPCHK(hipGetLastError());
    }
    return PCS_OK;
}

extern "C" {   // the public handle-free entries
int64_t pcs_dense_spd_work_len(int64_t n) {   // launch-per-column form: inverses + diagonal tiles + y; one-launch form: flags + x + y
    if (n <= 0) return -1;
    const int64_t nb = (n + 31) / 32;
    return std::max<int64_t>(2 * nb * 32 * 32 + nb * 32, cp_work_doubles(nb));
}

int pcs_dense_spd_solve_algo(int device, int64_t n, double *d_S, int64_t ld, const double *d_rhs, double *d_x, double *d_work, int32_t *d_status, void *stream,
                             int algorithm) {
    return enqueue_dense_spd(device, n, SpdSystem{d_S, ld, d_rhs, d_x, d_work, d_status}, SpdOptions{algorithm}, stream);
}

int pcs_dense_spd_solve(int device, int64_t n, double *d_S, int64_t ld, const double *d_rhs, double *d_x, double *d_work, int32_t *d_status, void *stream) {
    return pcs_dense_spd_solve_algo(device, n, d_S, ld, d_rhs, d_x, d_work, d_status, stream, PCS_SPD_AUTO);
}

int pcs_dense_spd_solve_opts(int device, int64_t n, double *d_S, int64_t ld, const double *d_rhs, double *d_x, double *d_work, int32_t *d_status, void *stream,
                             int algorithm, int64_t timeout_us) {
    if (timeout_us < 1 || timeout_us > 60000000) return fail(PCS_ERR_ARG, "pcs_dense_spd_solve_opts: timeout_us must be in [1, 60000000]");
    return enqueue_dense_spd(device, n, SpdSystem{d_S, ld, d_rhs, d_x, d_work, d_status}, SpdOptions{algorithm, nullptr, false, timeout_us}, stream);
}

int64_t pcs_schur_syrk_work_len(int64_t n_lead, int64_t n_trail) {
    if (n_lead <= 0 || n_trail < 0) return -1;
    return syrk_work_doubles(n_lead, n_trail);
}

static int schur_syrk_entry(const char *who, int device, int64_t n_lead, int64_t n_trail, const SyrkOperands &m, bool ordered, void *stream) {
    if (n_lead <= 0 || n_lead > (1 << 15) || n_trail < 0 || n_trail > (1ll << 30) || m.ldv < n_trail || m.lds < n_lead || !m.S || (n_trail && !m.V) || (m.u && !m.rhs) || (ordered && !m.ws))
        return fail(PCS_ERR_ARG, "%s: bad arguments", who);
    if (device < 0 || device >= pcs_device_count()) return fail(PCS_ERR_NODEVICE, "%s: device %d not available", who, device);
    if (n_trail == 0) return PCS_OK;
    HIPCHK(hipSetDevice(device));
    return enqueue_schur_syrk(n_lead, n_trail, m, (hipStream_t)stream, nullptr);
}
int pcs_schur_syrk_ordered(int device, int64_t n_lead, int64_t n_trail, const double *d_V, int64_t ldv, double *d_S, int64_t lds, const double *d_u,
                           double *d_rhs, double *d_work, int64_t work_doubles, void *stream) {
    return schur_syrk_entry("pcs_schur_syrk_ordered", device, n_lead, n_trail, SyrkOperands{d_V, ldv, d_S, lds, d_u, d_rhs, d_work, work_doubles}, true, stream);
}
int pcs_schur_syrk(int device, int64_t n_lead, int64_t n_trail, const double *d_V, int64_t ldv, double *d_S, int64_t lds, const double *d_u,
                   double *d_rhs, void *stream) {
    return schur_syrk_entry("pcs_schur_syrk", device, n_lead, n_trail, SyrkOperands{d_V, ldv, d_S, lds, d_u, d_rhs}, false, stream);
}

int pcs_schur_vtx(int device, int64_t n_lead, int64_t n_trail, const double *d_V, int64_t ldv, const double *d_x, double *d_w, void *stream) {
    if (n_lead <= 0 || n_trail < 0 || n_trail > (1ll << 30) || ldv < n_trail || (n_trail && (!d_V || !d_x || !d_w))) return fail(PCS_ERR_ARG, "pcs_schur_vtx: bad arguments");
    if (device < 0 || device >= pcs_device_count()) return fail(PCS_ERR_NODEVICE, "pcs_schur_vtx: device %d not available", device);
    if (n_trail == 0) return PCS_OK;
    HIPCHK(hipSetDevice(device));
    launch_schur_vtx(d_V, d_x, d_w, (int)n_lead, (int)n_trail, (int)ldv, nullptr, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}

int pcs_cov_trsm(int device, int64_t n, const double *d_L, int64_t ldl, double *d_X, int64_t n_rhs, int64_t ldx, int flags, void *stream) {
    const bool identity = (flags & PCS_COV_TRSM_IDENTITY) != 0;
    if (n <= 0 || n > (1 << 15) || n_rhs <= 0 || n_rhs > (1ll << 30) || ldl < n || ldx < n_rhs || !d_L || !d_X || (flags & ~PCS_COV_TRSM_IDENTITY) ||
        (identity && n_rhs != n) || n * ldx > (1ll << 40))
        return fail(PCS_ERR_ARG, "pcs_cov_trsm: bad arguments");
    if (device < 0 || device >= pcs_device_count()) return fail(PCS_ERR_NODEVICE, "pcs_cov_trsm: device %d not available", device);
    HIPCHK(hipSetDevice(device));
    const CovTrsmArgs a{d_L, d_X, ldl, ldx, (int32_t)n, (int32_t)n_rhs, identity ? 1 : 0};
    hipLaunchKernelGGL(cov_trsm_kernel, dim3((unsigned)((n_rhs + COV_NB - 1) / COV_NB)), dim3(256), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}

int pcs_cov_block_gram(int device, const double *d_X, int64_t ldx, int64_t n_rows, int64_t n_cols, const int32_t *d_col, const int32_t *d_width,
                       const int32_t *d_row0, int64_t n_blocks, double *d_out, int64_t out_stride, const double *d_linvt, int64_t tb,
                       const uint8_t *d_fixed, int64_t fixed_off, const double *d_scale, double scale, void *stream) {
    if (n_rows <= 0 || n_rows > (1ll << 30) || n_cols <= 0 || n_cols > (1ll << 30) || ldx < n_cols || !d_X || !d_col || !d_width || n_blocks < 0 ||
        n_blocks > (1ll << 31) - 1 || (n_blocks && !d_out) || out_stride < 1 || (d_linvt && (tb < 1 || tb > COV_NB)) || fixed_off < 0 || !(scale == scale))
        return fail(PCS_ERR_ARG, "pcs_cov_block_gram: bad arguments");
    if (device < 0 || device >= pcs_device_count()) return fail(PCS_ERR_NODEVICE, "pcs_cov_block_gram: device %d not available", device);
    if (n_blocks == 0) return PCS_OK;
    HIPCHK(hipSetDevice(device));
    CovGramArgs a{};
    a.X = d_X; a.ldx = ldx; a.n_rows = (int32_t)n_rows; a.n_cols = (int32_t)n_cols; a.n_blocks = (int32_t)n_blocks;
    a.col = d_col; a.width = d_width; a.row0 = d_row0; a.out = d_out; a.out_stride = out_stride;
    a.linvt = d_linvt; a.tb = (int32_t)tb; a.fixed = d_fixed; a.fixed_off = fixed_off; a.scale_dev = d_scale; a.scale = scale;
    hipLaunchKernelGGL(cov_gram_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return PCS_OK;
}

}  // extern "C"
