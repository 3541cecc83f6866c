// pcs_genchain.inc — host side of generated chains (included last by pcs_engine.hip; uses pcs_common.inc, pcs_handle.inc, pcs_dettable.inc and pcs_solver.inc).
//
// A pcs_genchain owns a code object that pycamset_amd/chain_compiler.py compiled for ONE composition of the reference's function
// blocks (csrc/ba_generic.hpp), the detection table, one Rodrigues slab per rigid parameter group and output scratch.  It is the
// generic counterpart of pcs_engine for the evaluation path (residual, dense Jacobian, masked data), for the products a solver needs
// (ba_blockrow.hpp) and — round 5 — for the exact Levenberg-Marquardt step on the DENSE normal equations of the chain
// (ba_blockgram.hpp + the step kernels of ba_schur.hpp with an empty trailing group + the dense Cholesky): pcs_genchain_lm_trial.
// The blocked (Schur) form, the order-deterministic sums and sharding stay with the three hand-fused chains.
#include "ba_generic.hpp"
#include "ba_blockrow.hpp"
#include "ba_blockgram.hpp"
#include "ba_blockcheck.hpp"

struct pcs_genchain {
    int device = 0;
    int P = 0, uses_template = 0, n_groups = 0, n_user = 0;
    int dtype = PCS_F64;   // PCS_F64 | PCS_F32 (float measurements and outputs) | PCS_MIXED (double measurements, float outputs); arithmetic is FP64
    int64_t user_off[GENERIC_MAX_GROUPS] = {};
    int64_t n_params = 0, n_cams = 0, n_imgs = 0, n_keys = 0;
    int64_t group_off[GENERIC_MAX_GROUPS] = {};
    int32_t group_count[GENERIC_MAX_GROUPS] = {};
    int64_t intr_off = 0, point_off = 0;
    hipModule_t module = nullptr;
    bool one_launch = true, prep_timed = false;
    bool two_pair_tiles = false;   // every 64-detection tile of the table lies inside a run of one (camera, image) pair or across one run boundary
    hipFunction_t f_prep = nullptr, f_eval[2][4] = {}, f_eval_f32[2][4] = {}, f_compact[2][4] = {}, f_compact_f32[2][4] = {};   // [one-launch form][mode]
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {};
    bool timed = false;
    DevBuf d_param, d_tmpl, d_slab[GENERIC_MAX_GROUPS];
    DevBuf d_sink;
    DetStore det;                   // the detection table (pcs_dettable.inc); det.n = number of detections
    PriorStore prior;               // the Gaussian parameter prior (pcs_genchain_set_prior); the handle's, not the table's
    BoundStore bounds;              // the box bounds of the LM solve (pcs_genchain_set_bounds); the handle's, not the table's
    bool have_template = false;
    DevBuf d_resid, d_jac, d_data;
    DevBuf d_keep;      // per detection, uint64: bit j set = local column j is free
    DevBuf d_row_off;   // per detection, int64: offset of its u row in the CSR data array
    int64_t nnz = -1;
    // products with the materialised Jacobian (pcs_genchain_linearize / pcs_genchain_matfree)
    int n_blocks = 0;
    int32_t blk_col0[BLOCKROW_MAX_BLOCKS] = {}, blk_np[BLOCKROW_MAX_BLOCKS] = {}, blk_link[BLOCKROW_MAX_BLOCKS] = {};
    int64_t blk_start[BLOCKROW_MAX_BLOCKS] = {};
    // shared parameter groups (pcs_genchain_set_group_maps): per block the table entity -> group index on the device (empty: the entity
    // itself) and how many groups it addresses; map_* are the same tables by the role the generated kernel reads them in
    int n_map_blocks = 0;
    bool any_map = false, evaluated = false;
    unsigned mapped_mask = 0;   // the code object's pcs_genchain_mapped: which groups its kernels index through a table
    DevBuf d_blk_map[BLOCKROW_MAX_BLOCKS];
    int32_t map_link[BLOCKROW_MAX_BLOCKS] = {}, map_groups[BLOCKROW_MAX_BLOCKS] = {};
    const int32_t *slab_map[GENERIC_MAX_GROUPS] = {}, *intr_map = nullptr, *point_map = nullptr, *user_map[GENERIC_MAX_GROUPS] = {};
    const int32_t *blk_map(int b) const { return b < n_map_blocks ? static_cast<const int32_t *>(d_blk_map[b].p) : nullptr; }
    int64_t blk_count(int b) const {   // parameter sets of block b: groups of a shared block, entities otherwise
        if (blk_map(b)) return map_groups[b];
        return blk_link[b] == 0 ? n_cams : blk_link[b] == 1 ? n_imgs : n_keys;
    }
    bool linearized = false;
    DevBuf d_vin, d_vout;   // max(n_params, 2N) + 1 doubles each
    // normal equations (ba_blockgram.hpp): per pass — (camera, image) = the table's order, (camera, key), (image, key) — the detections
    // in that order (passes 1, 2: an index per position) cut into segments; built on first use from the host copy of the index columns
    struct GramTables {   // one set per mode ([0] default, [1] ORDERED): switching the mode back and forth (a sharded solve does) rebuilds nothing
        int32_t *d_seg[4] = {}, *d_order[4] = {}, *d_grp[4][3] = {}, *d_gidx[4] = {};
        int64_t n_seg[4] = {}, n_grp[4][3] = {};
        bool built = false;
    } gram[2];
    // ORDERED mode (option "deterministic"): four orders, the groups of consecutive segments per order, a workspace of one matrix per segment
    bool deterministic = false, gram_keys = false;
    DevBuf d_gram_ws;
    int64_t spd_timeout_us = 250000;   // option "spd_timeout_us": how long the one-launch dense solve of an LM trial waits for a hand-over
    bool timing = true;                // option "timing": 0 = no start / stop events around the evaluation launches (an LM loop switches them off)
    int gram_debug = 0;                // option "gram_debug" (measurements only): 1 = no flush, 2 = no contraction
    // the blocked form of the normal equations (pcs_genchain_set_blocks decides): the LAST parameter group as ba_schur.hpp's trailing entities
    int64_t trail_off = -1, n_ent = 0;  // trail_off < 0: dense
    int tb = 3;
    bool dense_normal = false;          // option "dense_normal": 1 = the dense form whatever the chain
    size_t out_elem() const { return dtype == PCS_F64 ? sizeof(double) : sizeof(float); }
    int n_cu = 256;
};

extern "C" {

int pcs_genchain_destroy(pcs_genchain *h) {
    if (!h) return PCS_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->det.release();
    h->prior.release();
    h->bounds.release();
    for (DevBuf *b : {&h->d_param, &h->d_tmpl, &h->d_sink, &h->d_resid, &h->d_jac, &h->d_data, &h->d_keep, &h->d_row_off, &h->d_vin, &h->d_vout, &h->d_gram_ws}) b->release();
    for (DevBuf &b : h->d_slab) b.release();
    for (DevBuf &b : h->d_blk_map) b.release();
    for (auto &g : h->gram)
        for (int q = 0; q < 4; ++q)
            for (int32_t *b : {g.d_seg[q], g.d_order[q], g.d_grp[q][0], g.d_grp[q][1], g.d_grp[q][2], g.d_gidx[q]})
                if (b) (void)hipFree(b);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->module) (void)hipModuleUnload(h->module);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return PCS_OK;
}

int pcs_genchain_create(pcs_genchain **out, const char *code_object_path, int row_len, int uses_template, int n_groups, const int64_t *group_off,
                     const int32_t *group_count, int n_user, const int64_t *user_off, int64_t intr_off, int64_t point_off, int64_t n_params, int64_t n_cams,
                     int64_t n_imgs, int64_t n_keys, int dtype, int device) {
    if (!out || !code_object_path || row_len < 1 || row_len > 64 || n_groups < 0 || n_groups > GENERIC_MAX_GROUPS || (n_groups > 0 && (!group_off || !group_count)) ||
        n_user < 0 || n_user > GENERIC_MAX_GROUPS || (n_user > 0 && !user_off) || n_params <= 0 || n_cams <= 0 || n_imgs <= 0 || n_keys <= 0 ||
        (dtype != PCS_F64 && dtype != PCS_F32 && dtype != PCS_MIXED))
        return fail(PCS_ERR_ARG, "pcs_genchain_create: bad arguments");
    *out = nullptr;
    if (const int rc = open_device("pcs_genchain_create", device, "generated chains have no CPU fallback", true)) return rc;
    pcs_genchain *h = new pcs_genchain();
    h->device = device;
    h->uses_template = uses_template ? 1 : 0; h->n_groups = n_groups; h->n_user = n_user; h->dtype = dtype;
    h->P = row_len;
    h->n_params = n_params; h->n_cams = n_cams; h->n_imgs = n_imgs; h->n_keys = n_keys;
    h->intr_off = intr_off; h->point_off = point_off;
    for (int g = 0; g < n_groups; ++g) { h->group_off[g] = group_off[g]; h->group_count[g] = group_count[g]; }
    for (int u = 0; u < n_user; ++u) h->user_off[u] = user_off[u];
    // the steps of the set-up in order; the first that fails is named in the error and ends it
    hipError_t e = hipSuccess;
    std::string failed;
    auto step = [&](const std::string &what, hipError_t r) {
        if (r != hipSuccess) e = r, failed = what;
        return r == hipSuccess;
    };
    hipDeviceProp_t prop;
    bool ok = step("hipGetDeviceProperties", hipGetDeviceProperties(&prop, device));
    if (ok) {
        h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        ok = step(std::string("hipModuleLoad(") + code_object_path + ")", hipModuleLoad(&h->module, code_object_path));
    }
    auto function = [&](hipFunction_t *f, const std::string &name) { ok = ok && step("hipModuleGetFunction(" + name + ")", hipModuleGetFunction(f, h->module, name.c_str())); };
    function(&h->f_prep, "pcs_genchain_prep");
    for (int one = 0; one < 2; ++one) {
        const std::string sfx = one ? "_one" : "";
        for (int m = 1; m <= 3; ++m) {
            function(&h->f_eval[one][m], "pcs_genchain_eval_" + std::to_string(m) + sfx);
            function(&h->f_eval_f32[one][m], "pcs_genchain_eval_" + std::to_string(m) + "_f32" + sfx);
            if (m >= 2) {
                function(&h->f_compact[one][m], "pcs_genchain_compact_" + std::to_string(m) + sfx);
                function(&h->f_compact_f32[one][m], "pcs_genchain_compact_" + std::to_string(m) + "_f32" + sfx);
            }
        }
    }
    if (ok) {   // which parameter groups the code indexes through a table (shared parameters): pcs_genchain_set_group_maps must supply them
        hipDeviceptr_t d_mask = nullptr;
        size_t mask_bytes = 0;
        ok = step("hipModuleGetGlobal(pcs_genchain_mapped)", hipModuleGetGlobal(&d_mask, &mask_bytes, h->module, "pcs_genchain_mapped"));
        ok = ok && step("the size of pcs_genchain_mapped", mask_bytes == sizeof(unsigned) ? hipSuccess : hipErrorInvalidValue);
        ok = ok && step("hipMemcpyDtoH(pcs_genchain_mapped)", hipMemcpyDtoH(&h->mapped_mask, d_mask, sizeof(unsigned)));
    }
    ok = ok && step("hipStreamCreateWithFlags", hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (auto &ev : h->ev) ok = ok && step("hipEventCreate", hipEventCreate(&ev));
    ok = ok && step("hipMalloc(d_param)", h->d_param.alloc(n_params, sizeof(double)));
    ok = ok && step("hipMalloc(d_sink)", h->d_sink.alloc(8, sizeof(double)));   // 64 B
    for (int g = 0; g < n_groups; ++g) ok = ok && step("hipMalloc(d_slab)", h->d_slab[g].alloc(std::max<int64_t>(1, group_count[g]) * POSE_STRIDE, sizeof(double)));
    if (uses_template) ok = ok && step("hipMalloc(d_tmpl)", h->d_tmpl.alloc(3 * n_keys, sizeof(double)));
    if (!ok) {
        const int rc = fail(PCS_ERR_HIP, "%s failed: %s (pcs_genchain_create)", failed.c_str(), hipGetErrorString(e));
        pcs_genchain_destroy(h);
        return rc;
    }
    *out = h;
    return PCS_OK;
}

int pcs_genchain_row_len(const pcs_genchain *h) { return h ? h->P : -1; }

int pcs_genchain_set_detections_table(pcs_genchain *h, const double *det5, int64_t n) {
    if (!h || (!det5 && n > 0) || n < 0) return fail(PCS_ERR_ARG, "pcs_genchain_set_detections_table: bad arguments");
    const DetCounts counts{h->n_cams, h->n_imgs, h->n_keys, false};
    DetColumns c;
    std::vector<double> uv;
    if (const int rc = det_parse(det5, n, c, uv, &counts)) return rc;
    // the one-launch form's condition: every detection of a tile belongs to the (camera, image) pair of the tile's first or of its last detection
    h->two_pair_tiles = true;
    for (int64_t t0 = 0; t0 < n && h->two_pair_tiles; t0 += TILE) {
        const int64_t t1 = std::min<int64_t>(n, t0 + TILE) - 1;
        for (int64_t i = t0 + 1; i < t1; ++i)
            if ((c.cam[i] != c.cam[t0] || c.img[i] != c.img[t0]) && (c.cam[i] != c.cam[t1] || c.img[i] != c.img[t1])) { h->two_pair_tiles = false; break; }
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->det.release();   // det.n stays 0 (= "no detections set") if an allocation or copy below fails
    for (DevBuf *b : {&h->d_resid, &h->d_jac, &h->d_data, &h->d_keep, &h->d_row_off, &h->d_vin, &h->d_vout}) b->release();
    h->gram[0].built = h->gram[1].built = false;   // (the tables themselves are freed and rebuilt by genchain_gram_tables)
    h->linearized = false;
    h->nnz = -1;
    if (n == 0) return PCS_OK;
    if (const int rc = h->d_resid.grow(2 * n, h->out_elem())) return rc;
    if (const int rc = h->d_jac.grow(2 * n * h->P, h->out_elem())) return rc;
    return h->det.upload(c, uv.data(), counts, true, h->dtype == PCS_F32);   // generated chains always pack when the widths allow
}

int pcs_genchain_set_template(pcs_genchain *h, const double *points) {
    if (!h || !points) return fail(PCS_ERR_ARG, "pcs_genchain_set_template: bad arguments");
    if (!h->uses_template) return fail(PCS_ERR_ARG, "pcs_genchain_set_template: the chain's source is not template_points");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->d_tmpl.p, points, sizeof(double) * 3 * h->n_keys, hipMemcpyHostToDevice));
    h->have_template = true;
    return PCS_OK;
}

// slab preparation + evaluation at the device-resident parameter string; outputs in device memory (elements of the handle's dtype).
// compact: d_jac is the CSR data array and only the unfixed columns are written (pcs_genchain_set_unfixed).
static int genchain_enqueue(pcs_genchain *h, const double *d_param_str, void *d_resid, void *d_jac, bool compact, void *stream) {
    if (!h || !d_param_str) return fail(PCS_ERR_ARG, "pcs_genchain_eval_device: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    if (h->uses_template && !h->have_template) return fail(PCS_ERR_STATE, "template points not set");
    if (compact && (h->nnz < 0 || !d_jac)) return fail(PCS_ERR_STATE, "pcs_genchain_set_unfixed has not been called");
    if (h->any_map && h->n_blocks == 0) return fail(PCS_ERR_STATE, "pcs_genchain_set_group_maps was called: pcs_genchain_set_blocks must follow before the first evaluation");
    if (h->mapped_mask) {   // the kernels read these tables unconditionally
        bool have = (!(h->mapped_mask & 1u) || h->intr_map) && (!(h->mapped_mask & 2u) || h->point_map);
        for (int g = 0; g < GENERIC_MAX_GROUPS; ++g)
            have = have && (!((h->mapped_mask >> (8 + g)) & 1u) || h->slab_map[g]) && (!((h->mapped_mask >> (16 + g)) & 1u) || h->user_map[g]);
        if (!have) return fail(PCS_ERR_STATE, "the chain was compiled with shared parameter groups: pcs_genchain_set_group_maps and pcs_genchain_set_blocks must supply their tables first");
    }
    const int mode = (d_resid ? MODE_RESID : 0) | (d_jac ? MODE_JAC : 0);
    if (!mode) return PCS_OK;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    GenericArgs a{};
    a.tab = h->det.table();
    a.prm = d_param_str; a.tmpl = h->d_tmpl.as<double>();
    int64_t prep_threads = 0;
    for (int g = 0; g < h->n_groups; ++g) {
        a.slab[g] = h->d_slab[g].as<double>(); a.group_off[g] = h->group_off[g]; a.group_count[g] = h->group_count[g];
        prep_threads += (int64_t)h->group_count[g] * POSE_STRIDE;
    }
    a.n_groups = h->n_groups;
    a.intr_off = h->intr_off; a.point_off = h->point_off;
    for (int u = 0; u < h->n_user; ++u) { a.user_off[u] = h->user_off[u]; a.user_map[u] = h->user_map[u]; }
    for (int g = 0; g < h->n_groups; ++g) a.slab_map[g] = h->slab_map[g];
    a.intr_map = h->intr_map; a.point_map = h->point_map;
    h->evaluated = true;
    a.resid = d_resid; a.jac = d_jac; a.sink = h->d_sink.p;
    a.keep = h->d_keep.as<uint64_t>(); a.row_off = h->d_row_off.as<int64_t>();
    a.n = h->det.n; a.n_tiles = (h->det.n + TILE - 1) / TILE;
    const int waves = a.n_tiles >= (int64_t)h->n_cu * 32 ? WAVES_PER_WG : a.n_tiles >= (int64_t)h->n_cu * 16 ? 2 : 1;
    a.tiles_per_wg = waves;   // one tile per wave, like the hand-fused kernel with slabs through L1/L2
    void *params[] = {&a};
    // one launch per step when the table allows it (the reference's order does, unless a (camera, image) pair has fewer than ~32
    // detections); other tables take the form with prepared slabs and per-lane loads
    const int one = h->one_launch && h->two_pair_tiles && h->n_groups > 0 ? 1 : 0;
    const bool prep = prep_threads > 0 && !one;
    h->prep_timed = prep && h->timing;
    if (prep) HIPCHK(hipExtModuleLaunchKernel(h->f_prep, (uint32_t)((prep_threads + 63) / 64 * 64), 1, 1, 64, 1, 1, 0, s, params, nullptr, h->timing ? h->ev[0] : nullptr,
                                              h->timing ? h->ev[1] : nullptr, 0));
    const size_t esz = h->out_elem();
    const bool f32 = h->dtype != PCS_F64;
    size_t lds = 0;
    hipFunction_t f;
    if (compact) {
        const int vs = (int)(16 / esz), line = (int)(128 / esz);
        const int wave_lds = (HALF * 2 * h->P + line + 64 + vs - 1) / vs * vs;   // generic_compact_body's WAVE_LDS, rounded to 16-byte units
        lds = esz * (size_t)waves * wave_lds;
        f = f32 ? h->f_compact_f32[one][mode | MODE_JAC] : h->f_compact[one][mode | MODE_JAC];
    } else {
        lds = (mode & MODE_JAC) ? esz * (size_t)waves * HALF * lds_row_stride(2 * h->P, (int)esz) : 0;
        f = f32 ? h->f_eval_f32[one][mode] : h->f_eval[one][mode];
    }
    const int64_t grid = (a.n_tiles + waves - 1) / waves;
    HIPCHK(hipExtModuleLaunchKernel(f, (uint32_t)(grid * 64 * waves), 1, 1, 64 * waves, 1, 1, lds, s, params, nullptr, h->timing ? h->ev[2] : nullptr,
                                    h->timing ? h->ev[3] : nullptr, 0));
    if (h->timing) h->timed = true;
    return PCS_OK;
}

// 1 (the default): a step is ONE launch — every wave prepares the Rodrigues slabs of its tile's (camera, image) pairs itself — for
// tables whose 64-detection tiles lie inside a run of one pair or across one run boundary (the reference's table order); 0, and
// other tables: slab preparation as a launch of its own in front of the evaluation.  Same bits either way.
int pcs_genchain_set_one_launch(pcs_genchain *h, int on) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_set_one_launch: null handle");
    h->one_launch = on != 0;
    return PCS_OK;
}

int pcs_genchain_eval_device(pcs_genchain *h, const double *d_param_str, void *d_resid, void *d_jac, void *stream) {
    return genchain_enqueue(h, d_param_str, d_resid, d_jac, false, stream);
}

// residual (optional) + ONLY the unfixed columns of the Jacobian, in CSR data order, at the device-resident parameter string
int pcs_genchain_eval_compact_device(pcs_genchain *h, const double *d_param_str, void *d_resid, void *d_data, void *stream) {
    if (!d_data) return fail(PCS_ERR_ARG, "pcs_genchain_eval_compact_device: bad arguments");
    return genchain_enqueue(h, d_param_str, d_resid, d_data, true, stream);
}

static int chain_stage(pcs_genchain *h, const double *param_str) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpyAsync(h->d_param.as<double>(), param_str, sizeof(double) * h->n_params, hipMemcpyHostToDevice, h->stream));
    return PCS_OK;
}

int pcs_genchain_eval(pcs_genchain *h, const double *param_str, void *resid, void *jac) {
    if (!h || !param_str) return fail(PCS_ERR_ARG, "pcs_genchain_eval: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    int rc = chain_stage(h, param_str);
    if (rc) return rc;
    rc = pcs_genchain_eval_device(h, h->d_param.as<double>(), resid ? h->d_resid.p : nullptr, jac ? h->d_jac.p : nullptr, nullptr);
    if (rc) return rc;
    if (resid) HIPCHK(hipMemcpyAsync(resid, h->d_resid.p, h->out_elem() * 2 * h->det.n, hipMemcpyDeviceToHost, h->stream));
    if (jac) HIPCHK(hipMemcpyAsync(jac, h->d_jac.p, h->out_elem() * 2 * h->det.n * h->P, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PCS_OK;
}

// The fixed-parameter mask as per-detection tables (afb:465-489 resolved per block row): keep[i] bit j = local column j of detection i
// is free; row_off[i] = offset of its u row in the CSR data array (its v row follows: same kept columns).  nnz = total entries.
int pcs_genchain_set_unfixed(pcs_genchain *h, const uint64_t *keep, const int64_t *row_off, int64_t nnz) {
    if (!h || nnz < 0 || !keep || !row_off) return fail(PCS_ERR_ARG, "pcs_genchain_set_unfixed: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    int64_t expect = 0;
    for (int64_t i = 0; i < h->det.n; ++i) {
        if (h->P < 64 && (keep[i] >> h->P)) return fail(PCS_ERR_RANGE, "pcs_genchain_set_unfixed: detection %lld keeps a column beyond the row length", (long long)i);
        if (row_off[i] != expect) return fail(PCS_ERR_RANGE, "pcs_genchain_set_unfixed: row_off[%lld] = %lld, the packed layout needs %lld", (long long)i, (long long)row_off[i], (long long)expect);
        expect += 2 * (int64_t)__builtin_popcountll(keep[i]);
    }
    if (expect != nnz) return fail(PCS_ERR_RANGE, "pcs_genchain_set_unfixed: nnz = %lld, the masks keep %lld entries", (long long)nnz, (long long)expect);
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (DevBuf *b : {&h->d_keep, &h->d_row_off, &h->d_data}) b->release();
    if (const int rc = h->d_keep.grow(h->det.n, sizeof(uint64_t))) return rc;
    if (const int rc = h->d_row_off.grow(h->det.n, sizeof(int64_t))) return rc;
    if (const int rc = h->d_data.grow((int64_t)h->out_elem() * std::max<int64_t>(1, nnz) + 256, 1)) return rc;   // bytes; + one line: the last pass may store whole 16-byte units
    HIPCHK(hipMemcpy(h->d_keep.p, keep, sizeof(uint64_t) * h->det.n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_row_off.p, row_off, sizeof(int64_t) * h->det.n, hipMemcpyHostToDevice));
    h->nnz = nnz;
    return PCS_OK;
}

int pcs_genchain_eval_compact(pcs_genchain *h, const double *param_str, void *resid, void *data) {
    if (!h || !param_str || !data) return fail(PCS_ERR_ARG, "pcs_genchain_eval_compact: bad arguments");
    if (h->nnz < 0) return fail(PCS_ERR_STATE, "pcs_genchain_set_unfixed has not been called");
    int rc = chain_stage(h, param_str);
    if (rc) return rc;
    rc = genchain_enqueue(h, h->d_param.as<double>(), resid ? h->d_resid.p : nullptr, h->d_data.p, true, nullptr);
    if (rc) return rc;
    if (h->nnz > 0) HIPCHK(hipMemcpyAsync(data, h->d_data.p, h->out_elem() * h->nnz, hipMemcpyDeviceToHost, h->stream));
    if (resid) HIPCHK(hipMemcpyAsync(resid, h->d_resid.p, h->out_elem() * 2 * h->det.n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PCS_OK;
}

// Shared parameter groups (param_type's mod_function / key_type.SINGLE; the reference declares them, afb:42-61, and leaves them a TODO,
// afb:803): per block a table entity -> group index, NULL for a block indexed by the entity itself.  Called once, after create and BEFORE
// pcs_genchain_set_blocks (which then counts a shared block's parameter sets in groups) and before the first evaluation; nothing is
// launched.  table_len[b] must be the entity count of link[b] given at create, every value lie in [0, n_mapped[b]).
int pcs_genchain_set_group_maps(pcs_genchain *h, int n_blocks, const int32_t *link, const int32_t *const *tables, const int64_t *table_len, const int32_t *n_mapped) {
    if (!h || n_blocks < 1 || n_blocks > BLOCKROW_MAX_BLOCKS || !link || !tables || !table_len || !n_mapped) return fail(PCS_ERR_ARG, "pcs_genchain_set_group_maps: bad arguments");
    if (h->evaluated) return fail(PCS_ERR_ARG, "pcs_genchain_set_group_maps: the chain has been evaluated; the tables are set once, before the first evaluation");
    if (h->n_blocks != 0 || h->any_map) return fail(PCS_ERR_ARG, "pcs_genchain_set_group_maps: call it once, before pcs_genchain_set_blocks");
    bool any = false;
    for (int b = 0; b < n_blocks; ++b) {
        if (!tables[b]) continue;
        any = true;
        const int64_t count = link[b] == 0 ? h->n_cams : link[b] == 1 ? h->n_imgs : link[b] == 2 ? h->n_keys : -1;
        if (count < 0) return fail(PCS_ERR_ARG, "pcs_genchain_set_group_maps: block %d has link %d (0 camera, 1 image, 2 key)", b, link[b]);
        if (table_len[b] != count) return fail(PCS_ERR_ARG, "pcs_genchain_set_group_maps: the table of block %d has %lld entries, the chain has %lld entities of its link", b, (long long)table_len[b], (long long)count);
        if (n_mapped[b] < 1) return fail(PCS_ERR_RANGE, "pcs_genchain_set_group_maps: block %d maps to %d groups", b, n_mapped[b]);
        for (int64_t i = 0; i < count; ++i)
            if (tables[b][i] < 0 || tables[b][i] >= n_mapped[b])
                return fail(PCS_ERR_RANGE, "pcs_genchain_set_group_maps: table of block %d, entity %lld -> group %d outside [0, %d)", b, (long long)i, tables[b][i], n_mapped[b]);
    }
    if (!any) return PCS_OK;
    HIPCHK(hipSetDevice(h->device));
    for (int b = 0; b < n_blocks; ++b) {
        if (!tables[b]) continue;
        hipError_t e = h->d_blk_map[b].alloc(table_len[b], sizeof(int32_t));
        if (e == hipSuccess) e = hipMemcpy(h->d_blk_map[b].p, tables[b], sizeof(int32_t) * table_len[b], hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            for (DevBuf &m : h->d_blk_map) m.release();
            return fail(PCS_ERR_HIP, "pcs_genchain_set_group_maps: uploading the table of block %d failed: %s", b, hipGetErrorString(e));
        }
        h->map_link[b] = link[b]; h->map_groups[b] = n_mapped[b];
    }
    h->n_map_blocks = n_blocks; h->any_map = true;
    return PCS_OK;
}

// Which global column every local column of a block row stands for (the reference's get_block_param_inds, afb:192-233, as a rule):
// block b covers local columns [col0_b, col0_b + np_b), its parameters of entity e (camera / image / key by link_b) start at
// start_b + np_b e.  Needed by pcs_genchain_matfree only.
int pcs_genchain_set_blocks(pcs_genchain *h, int n_blocks, const int32_t *col0, const int32_t *n_params, const int32_t *link, const int64_t *start) {
    if (!h || n_blocks < 1 || n_blocks > BLOCKROW_MAX_BLOCKS || !col0 || !n_params || !link || !start) return fail(PCS_ERR_ARG, "pcs_genchain_set_blocks: bad arguments");
    if (h->any_map && n_blocks != h->n_map_blocks)
        return fail(PCS_ERR_ARG, "pcs_genchain_set_blocks: %d blocks, pcs_genchain_set_group_maps described %d", n_blocks, h->n_map_blocks);
    int64_t cols = 0;
    for (int b = 0; b < n_blocks; ++b) {
        int64_t count = link[b] == 0 ? h->n_cams : link[b] == 1 ? h->n_imgs : link[b] == 2 ? h->n_keys : -1;
        if (h->blk_map(b)) {   // a shared block: its group holds one parameter set per GROUP
            if (link[b] != h->map_link[b]) return fail(PCS_ERR_ARG, "pcs_genchain_set_blocks: block %d has link %d, its table was given for link %d", b, link[b], h->map_link[b]);
            count = h->map_groups[b];
        }
        if (count < 0 || col0[b] != cols || n_params[b] < 1 || start[b] < 0 || start[b] + n_params[b] * count > h->n_params)
            return fail(PCS_ERR_RANGE, "pcs_genchain_set_blocks: block %d does not fit the parameter string", b);
        cols += n_params[b];
    }
    if (cols != h->P) return fail(PCS_ERR_RANGE, "pcs_genchain_set_blocks: the blocks cover %lld columns, the row has %d", (long long)cols, h->P);
    for (int b = 0; b < n_blocks; ++b)   // blocks of ONE group (the same first column) go through the same table, or through none
        for (int c = b + 1; c < n_blocks; ++c)
            if (start[b] == start[c] && (h->blk_map(b) != nullptr) != (h->blk_map(c) != nullptr))
                return fail(PCS_ERR_ARG, "pcs_genchain_set_blocks: blocks %d and %d share a parameter group, but only one of them has a table (pcs_genchain_set_group_maps)", b, c);
            else if (start[b] == start[c] && h->blk_map(b) && h->map_groups[b] != h->map_groups[c])
                return fail(PCS_ERR_ARG, "pcs_genchain_set_blocks: blocks %d and %d share a parameter group, their tables address %d and %d groups", b, c, h->map_groups[b], h->map_groups[c]);
    h->n_blocks = n_blocks;
    h->gram[0].built = h->gram[1].built = false;
    for (int b = 0; b < n_blocks; ++b) { h->blk_col0[b] = col0[b]; h->blk_np[b] = n_params[b]; h->blk_link[b] = link[b]; h->blk_start[b] = start[b]; }
    // the tables by the role the generated kernel reads them in: a block's group is the rigid group, the intrinsics, the points or the
    // user block whose first column it starts at (a role the chain does not have is never read)
    for (int g = 0; g < GENERIC_MAX_GROUPS; ++g) h->slab_map[g] = h->user_map[g] = nullptr;
    h->intr_map = h->point_map = nullptr;
    for (int b = 0; b < n_blocks; ++b) {
        const int32_t *map = h->blk_map(b);
        if (!map) continue;
        for (int g = 0; g < h->n_groups; ++g)
            if (h->group_off[g] == start[b]) {
                if (h->group_count[g] != h->map_groups[b]) {
                    h->n_blocks = 0;
                    return fail(PCS_ERR_RANGE, "pcs_genchain_set_blocks: block %d maps to %d groups, its rigid group was created with %d", b, h->map_groups[b], h->group_count[g]);
                }
                h->slab_map[g] = map;
            }
        for (int u = 0; u < h->n_user; ++u)
            if (h->user_off[u] == start[b]) h->user_map[u] = map;
        if (h->intr_off == start[b]) h->intr_map = map;
        if (h->point_off == start[b]) h->point_map = map;
    }
    // Schur structure: the group that ENDS the parameter string, when it is one rigid transform per image (6) or one point per key (3) —
    // the entity kinds the step kernels of ba_schur.hpp factor in registers — and something leads it.  A detection has one image and one
    // key, so two such entities never share a row: C is block diagonal.  Every other chain keeps the dense form.
    h->trail_off = -1; h->n_ent = 0;
    int last = 0;
    for (int b = 1; b < n_blocks; ++b)
        if (start[b] > start[last]) last = b;
    const int64_t count = link[last] == 1 ? h->n_imgs : link[last] == 2 ? h->n_keys : h->n_cams;
    const bool kind = (n_params[last] == 6 && link[last] == 1) || (n_params[last] == 3 && link[last] == 2);
    bool alone = true;   // no other group overlaps it
    for (int b = 0; b < n_blocks; ++b)
        if (start[b] != start[last] && start[b] + (int64_t)n_params[b] * h->blk_count(b) > start[last]) alone = false;
    bool shared = false;   // a shared group is never the trailing group: its entities would not own their block of C
    for (int b = 0; b < n_blocks; ++b)
        if (start[b] == start[last] && h->blk_map(b)) shared = true;
    if (kind && alone && !shared && start[last] > 0 && start[last] + n_params[last] * count == h->n_params) {
        h->trail_off = start[last]; h->tb = n_params[last]; h->n_ent = count;
    }
    return PCS_OK;
}

// Evaluate residual + dense Jacobian at param_str into the handle's device buffers: the point pcs_genchain_matfree refers to.
int pcs_genchain_linearize(pcs_genchain *h, const double *param_str) {
    if (!h || !param_str) return fail(PCS_ERR_ARG, "pcs_genchain_linearize: bad arguments");
    if (h->dtype != PCS_F64) return fail(PCS_ERR_STATE, "pcs_genchain_linearize: the products read an FP64 Jacobian (create the chain with PCS_F64)");
    if (h->n_blocks == 0) return fail(PCS_ERR_STATE, "pcs_genchain_set_blocks has not been called");
    int rc = chain_stage(h, param_str);
    if (rc) return rc;
    rc = genchain_enqueue(h, h->d_param.as<double>(), h->d_resid.p, h->d_jac.p, false, nullptr);
    if (rc) return rc;
    h->linearized = true;
    return PCS_OK;
}

// op codes and vector shapes of pcs_matfree (host vectors, FULL parameter-string space)
int pcs_genchain_matfree(pcs_genchain *h, int op, const double *in, double *out, double *cost) {
    if (!h || !out || op < 0 || op > 4 || ((op == BR_JV || op == BR_JTU || op == BR_JTJV) && !in)) return fail(PCS_ERR_ARG, "pcs_genchain_matfree: bad arguments");
    if (!h->linearized) return fail(PCS_ERR_STATE, "pcs_genchain_linearize has not been called");
    HIPCHK(hipSetDevice(h->device));
    const int64_t n_in = op == BR_JTU ? 2 * h->det.n : (op == BR_JV || op == BR_JTJV) ? h->n_params : 0;
    const int64_t n_out = op == BR_JV ? 2 * h->det.n : h->n_params;
    const int64_t cap = std::max<int64_t>(h->n_params, 2 * h->det.n) + 1;
    if (const int rc = h->d_vin.grow(cap, sizeof(double))) return rc;   // released with the table: allocated once per table
    if (const int rc = h->d_vout.grow(cap, sizeof(double))) return rc;
    hipStream_t s = h->stream;
    if (n_in) HIPCHK(hipMemcpyAsync(h->d_vin.as<double>(), in, sizeof(double) * n_in, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(h->d_vout.as<double>(), 0, sizeof(double) * (n_out + 1), s));
    BlockRowArgs a{};
    a.tab = h->det.table();   // (FP64 chains only: double measurements)
    a.J = static_cast<const double *>(h->d_jac.p); a.resid = static_cast<const double *>(h->d_resid.p);
    a.in = h->d_vin.as<double>(); a.out = h->d_vout.as<double>(); a.cost = h->d_vout.as<double>() + n_out;
    a.n = h->det.n; a.n_params = h->n_params; a.P = h->P; a.n_blocks = h->n_blocks;
    for (int b = 0; b < h->n_blocks; ++b) { a.blk_col0[b] = h->blk_col0[b]; a.blk_np[b] = h->blk_np[b]; a.blk_link[b] = h->blk_link[b]; a.blk_start[b] = h->blk_start[b]; a.blk_map[b] = h->blk_map(b); }
    a.lds_acc = op != BR_JV && h->n_params * (int64_t)sizeof(double) <= 65536;
    const size_t lds = a.lds_acc ? sizeof(double) * (size_t)h->n_params : 0;
    const int64_t wgs = std::min<int64_t>((h->det.n + 255) / 256, (int64_t)h->n_cu * (a.lds_acc ? 2 : 8));
    const dim3 grid((unsigned)std::max<int64_t>(1, wgs));
    switch (op) {
        case BR_JV: hipLaunchKernelGGL(blockrow_kernel<BR_JV>, grid, dim3(256), lds, s, a); break;
        case BR_JTU: hipLaunchKernelGGL(blockrow_kernel<BR_JTU>, grid, dim3(256), lds, s, a); break;
        case BR_JTJV: hipLaunchKernelGGL(blockrow_kernel<BR_JTJV>, grid, dim3(256), lds, s, a); break;
        case BR_DIAG: hipLaunchKernelGGL(blockrow_kernel<BR_DIAG>, grid, dim3(256), lds, s, a); break;
        default: hipLaunchKernelGGL(blockrow_kernel<BR_GRAD>, grid, dim3(256), lds, s, a); break;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_vout.as<double>(), sizeof(double) * n_out, hipMemcpyDeviceToHost, s));
    if (cost && op == BR_GRAD) HIPCHK(hipMemcpyAsync(cost, h->d_vout.as<double>() + n_out, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PCS_OK;
}

// ---- dense normal equations and the exact Levenberg-Marquardt trial (round 5) -------------------------------------------------------
// The packed state of a generated chain is [A | g | cost] with A = J^T J dense (n_params x n_params, upper triangle written): the
// blocked layout of pcs_normal_layout with every parameter in the leading group and no trailing entities.
static BlockLayout genchain_layout(const pcs_genchain *h) {
    BlockLayout L{};
    L.tg = 0;
    if (h->trail_off > 0 && !h->dense_normal) {
        L.tb = h->tb; L.n_ent = h->n_ent; L.n_trail = h->n_ent * h->tb; L.n_lead = L.trail_off = h->trail_off;
    } else {
        L.tb = 3; L.n_ent = 0; L.n_trail = 0; L.n_lead = L.trail_off = h->n_params;
    }
    return L;
}

int pcs_genchain_normal_layout(const pcs_genchain *h, int64_t *out5) {
    if (!h || !out5) return fail(PCS_ERR_ARG, "pcs_genchain_normal_layout: bad arguments");
    layout_out5(genchain_layout(h), h->n_params, out5);
    return PCS_OK;
}

int pcs_genchain_set_option(pcs_genchain *h, const char *key, int64_t value) {
    if (!h || !key) return fail(PCS_ERR_ARG, "pcs_genchain_set_option: bad arguments");
    if (!strcmp(key, "spd_timeout_us")) {
        if (value < 1) return fail(PCS_ERR_ARG, "spd_timeout_us must be positive");
        h->spd_timeout_us = value;
    } else if (!strcmp(key, "timing")) {
        h->timing = value != 0;
    } else if (!strcmp(key, "gram_debug")) {
        h->gram_debug = (int)value;
    } else if (!strcmp(key, "dense_normal")) {
        h->dense_normal = value != 0;
    } else if (!strcmp(key, "deterministic")) {
        if (value && h->any_map) return fail(PCS_ERR_ARG, "deterministic mode: shared parameter groups (pcs_genchain_set_group_maps) are not supported in the ordered sums");
        if (value) {   // every destination must belong to ONE pair of local columns (blockrow_gram_reduce_kernel writes it with a plain add)
            for (int b = 0; b < h->n_blocks; ++b)
                for (int c = b + 1; c < h->n_blocks; ++c)
                    if (h->blk_start[b] == h->blk_start[c])
                        return fail(PCS_ERR_ARG, "deterministic mode: blocks %d and %d share a parameter group (two local columns per parameter are not supported in the ordered sums)", b, c);
        }
        h->deterministic = value != 0;
    } else {
        return fail(PCS_ERR_ARG, "pcs_genchain_set_option: unknown option '%s'", key);
    }
    return PCS_OK;
}

// Segment tables of the contraction (ba_blockgram.hpp).  Default mode: pass 0 (the table's own order: runs of one (camera, image) pair)
// always; passes 1 and 2 — (camera, key) and (image, key) order — when the chain has columns linked to the key.  ORDERED mode: the
// orders (camera, image) and — for chains with key columns — (key, camera), (image, key), every one SORTED (an index per position), and
// per order the groups of consecutive segments by its major entity and by (major, minor); in the (camera, image) order of a chain
// without key columns also each IMAGE's segments as a list (the image x image pairs are summed through it).  A run of equal entities is
// cut into equal pieces of at most `cap` detections: GRAM_SEG for big tables, shorter for small ones so that a few thousand waves exist
// (a wave walks its segment's rows in sequence: 7 005 detections as 72 runs of ~100 took 55 us, latency of 13 dependent load - contract
// rounds on 72 waves).
static int genchain_gram_tables(pcs_genchain *h) {
    pcs_genchain::GramTables &G = h->gram[h->deterministic ? 1 : 0];
    if (G.built) return PCS_OK;
    const int64_t n = h->det.n;
    if (n > INT32_MAX) return fail(PCS_ERR_ARG, "normal equations of the chain: tables beyond 2^31 rows are not supported");
    bool key_linked = false;
    for (int b = 0; b < h->n_blocks; ++b) key_linked = key_linked || h->blk_link[b] == 2;
    h->gram_keys = key_linked;
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int p = 0; p < 4; ++p)
        for (int32_t **b : {&G.d_seg[p], &G.d_order[p], &G.d_grp[p][0], &G.d_grp[p][1], &G.d_grp[p][2], &G.d_gidx[p]}) {   // (rebuilt after pcs_genchain_set_blocks / a new table)
            if (*b) HIPCHK(hipFree(*b));
            *b = nullptr;
        }
    for (int p = 0; p < 4; ++p) G.n_seg[p] = G.n_grp[p][0] = G.n_grp[p][1] = G.n_grp[p][2] = 0;
    const int64_t cap = std::min<int64_t>(GRAM_SEG, std::max<int64_t>(16, (n / 4096 + 15) / 16 * 16));
    const std::vector<int32_t> *kind[3] = {&h->det.h.cam, &h->det.h.img, &h->det.h.key};
    // (major, minor) entity kinds per pass; -1: the pass does not exist in this mode / for this chain
    int major[4] = {-1, -1, -1, -1}, minor[4] = {-1, -1, -1, -1};
    bool sorted[4] = {false, false, false, false};
    if (!h->deterministic) {
        major[0] = 0; minor[0] = 1;                                       // the table's own order: runs of (camera, image)
        if (key_linked) { major[1] = 0; minor[1] = 2; sorted[1] = true; major[2] = 1; minor[2] = 2; sorted[2] = true; }
    } else {
        major[0] = 0; minor[0] = 1; sorted[0] = true;
        // (without key columns the image x image pairs are summed from pass 0's workspace through a list of each image's segments)
        if (key_linked) { major[2] = 2; minor[2] = 0; sorted[2] = true; major[3] = 1; minor[3] = 2; sorted[3] = true; }
    }
    for (int pass = 0; pass < 4; ++pass) {
        if (major[pass] < 0) continue;
        const std::vector<int32_t> &x = *kind[major[pass]], &y = *kind[minor[pass]];
        std::vector<int32_t> order;
        if (sorted[pass]) {
            order.resize(n);
            for (int64_t i = 0; i < n; ++i) order[i] = (int32_t)i;
            std::stable_sort(order.begin(), order.end(), [&](int32_t p, int32_t q) { return x[p] != x[q] ? x[p] < x[q] : y[p] < y[q]; });
        }
        auto at = [&](int64_t pos) { return sorted[pass] ? (int64_t)order[pos] : pos; };
        std::vector<int32_t> seg, g0, g1;   // g0 / g1: groups by the major entity / by (major, minor): (first segment, one past the last)
        for (int64_t i = 0; i < n;) {
            const int64_t d = at(i);
            int64_t j = i + 1;
            while (j < n && x[at(j)] == x[d] && y[at(j)] == y[d]) ++j;
            const int64_t run = j - i, pieces = (run + cap - 1) / cap, len = (run + pieces - 1) / pieces;
            const int32_t s_first = (int32_t)(seg.size() / GRAM_SEG_WORDS);
            for (int64_t k = i; k < j; k += len) {
                int32_t ids[3] = {-1, -1, -1};
                ids[major[pass]] = x[d]; ids[minor[pass]] = y[d];
                seg.push_back((int32_t)k); seg.push_back((int32_t)std::min(len, j - k)); seg.push_back(ids[0]); seg.push_back(ids[1]); seg.push_back(ids[2]);
            }
            const int32_t s_end = (int32_t)(seg.size() / GRAM_SEG_WORDS);
            g1.push_back(s_first); g1.push_back(s_end);
            if (i > 0 && x[at(i - 1)] == x[d]) g0.back() = s_end;        // the major entity continues: extend its group
            else { g0.push_back(s_first); g0.push_back(s_end); }
            i = j;
        }
        auto upload = [&](int32_t **dst, const std::vector<int32_t> &v) -> hipError_t {
            hipError_t e = hipMalloc(dst, sizeof(int32_t) * std::max<size_t>(1, v.size()));
            return e != hipSuccess || v.empty() ? e : hipMemcpy(*dst, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice);
        };
        HIPCHK(upload(&G.d_seg[pass], seg));
        G.n_seg[pass] = (int64_t)seg.size() / GRAM_SEG_WORDS;
        if (sorted[pass]) HIPCHK(upload(&G.d_order[pass], order));
        if (h->deterministic) {
            HIPCHK(upload(&G.d_grp[pass][0], g0));
            HIPCHK(upload(&G.d_grp[pass][1], g1));
            G.n_grp[pass][0] = (int64_t)g0.size() / 2; G.n_grp[pass][1] = (int64_t)g1.size() / 2;
            if (pass == 0 && !key_linked) {   // groups by the MINOR entity (the image): each image's segments, in table order, through a list
                const int64_t ns = (int64_t)seg.size() / GRAM_SEG_WORDS;
                std::vector<int32_t> idx(ns), g2;
                for (int64_t q = 0; q < ns; ++q) idx[q] = (int32_t)q;
                std::stable_sort(idx.begin(), idx.end(), [&](int32_t p, int32_t q) { return seg[GRAM_SEG_WORDS * p + 3] < seg[GRAM_SEG_WORDS * q + 3]; });
                for (int64_t q = 0; q < ns;) {
                    int64_t r = q + 1;
                    while (r < ns && seg[GRAM_SEG_WORDS * idx[r] + 3] == seg[GRAM_SEG_WORDS * idx[q] + 3]) ++r;
                    g2.push_back((int32_t)q); g2.push_back((int32_t)r);
                    q = r;
                }
                HIPCHK(upload(&G.d_grp[pass][2], g2));
                HIPCHK(upload(&G.d_gidx[pass], idx));
                G.n_grp[pass][2] = (int64_t)g2.size() / 2;
            }
        }
    }
    G.built = true;
    return PCS_OK;
}

// evaluation at d_param_str into the handle's block rows, then their contraction into d_packed = [A | B | C | g | cost] (zeroed here)
static int genchain_enqueue_normal(pcs_genchain *h, const double *d_param_str, double *d_packed, hipStream_t s, const int32_t *d_stop, bool zeroed = false) {
    if (h->dtype != PCS_F64) return fail(PCS_ERR_STATE, "dense normal equations read an FP64 Jacobian (create the chain with PCS_F64)");
    if (h->n_blocks == 0) return fail(PCS_ERR_STATE, "pcs_genchain_set_blocks has not been called");
    if (h->P + 1 > GRAM_MAX_COLS) return fail(PCS_ERR_ARG, "dense normal equations: block rows of %d columns (limit %d)", h->P, GRAM_MAX_COLS - 1);
    if (h->n_params > PCS_NORMAL_MAX_PARAMS) return fail(PCS_ERR_ARG, "dense normal equations: more than %d parameters", PCS_NORMAL_MAX_PARAMS);
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    int rc = genchain_gram_tables(h);
    if (rc) return rc;
    const pcs_genchain::GramTables &G = h->gram[h->deterministic ? 1 : 0];
    rc = genchain_enqueue(h, d_param_str, h->d_resid.p, h->d_jac.p, false, s);
    if (rc) return rc;
    h->linearized = true;
    const int64_t np = h->n_params;
    const BlockLayout L = genchain_layout(h);
    const int64_t lim = (int64_t)1 << 32;
    if (L.a_len() >= lim || L.b_len() >= lim || L.c_len() >= lim) return fail(PCS_ERR_ARG, "normal equations of the chain: a region beyond 32 GiB");
    const int64_t n_h = L.h_len();
    if (!zeroed) HIPCHK(hipMemsetAsync(d_packed, 0, sizeof(double) * (size_t)(n_h + np + 1), s));
    BlockGramArgs a{};
    a.tab = h->det.table();   // (FP64 chains only: double measurements)
    a.J = static_cast<const double *>(h->d_jac.p); a.resid = static_cast<const double *>(h->d_resid.p);
    a.A = d_packed; a.B = a.A + L.a_len(); a.C = a.B + L.b_len(); a.g = d_packed + n_h; a.cost = a.g + np;
    a.n_params = np; a.n_lead = L.n_lead; a.n_trail = L.n_trail; a.trail_off = L.trail_off; a.tb = L.tb;
    a.P = h->P; a.n_blocks = h->n_blocks;
    for (int b = 0; b < h->n_blocks; ++b) { a.blk_col0[b] = h->blk_col0[b]; a.blk_np[b] = h->blk_np[b]; a.blk_link[b] = h->blk_link[b]; a.blk_start[b] = h->blk_start[b]; a.blk_map[b] = h->blk_map(b); }
    a.stop = d_stop; a.debug = h->gram_debug;
    const int nb = (h->P + 1 + 15) / 16;
    auto launch = [&](auto kernel, int nbc) -> hipError_t {
        const int waves = gram_waves(nbc);
        const size_t lds = sizeof(double) * (size_t)waves * gram_blocks(nbc) * 256;
        // more than 64 KB of dynamic LDS wants the attribute (set per launch: a handle may live on any device)
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((a.n_seg + waves - 1) / waves)), dim3(64 * waves), lds, s, a);
        return hipGetLastError();
    };
    if (h->deterministic) {   // the workspace of the ordered mode: one matrix per segment of the longest pass
        int64_t most = 0;
        for (int pass = 0; pass < 4; ++pass) most = std::max(most, G.n_seg[pass]);
        const int64_t need = most * gram_blocks(nb) * 256;
        if (h->d_gram_ws.grows(need)) {
            HIPCHK(hipStreamSynchronize(s));
            if (const int rc = h->d_gram_ws.grow(need, sizeof(double))) return rc;
        }
    }
    for (int pass = 0; pass < 4; ++pass) {   // one launch per table order that has pairs of columns to sum (default mode: key-linked columns add two)
        if (G.n_seg[pass] <= 0) continue;
        a.seg = G.d_seg[pass]; a.n_seg = (int32_t)G.n_seg[pass]; a.order = G.d_order[pass]; a.pass = pass;
        a.det = h->deterministic ? 1 : 0; a.ws = h->deterministic ? h->d_gram_ws.as<double>() : nullptr;
        a.grp[0] = G.d_grp[pass][0]; a.grp[1] = G.d_grp[pass][1]; a.grp[2] = G.d_grp[pass][2]; a.gidx = G.d_gidx[pass];
        a.n_grp[0] = (int32_t)G.n_grp[pass][0]; a.n_grp[1] = (int32_t)G.n_grp[pass][1]; a.n_grp[2] = (int32_t)G.n_grp[pass][2];
        hipError_t e;
        switch (nb) {
            case 1: e = launch(blockrow_gram_kernel<1>, 1); break;
            case 2: e = launch(blockrow_gram_kernel<2>, 2); break;
            case 3: e = launch(blockrow_gram_kernel<3>, 3); break;
            default: e = launch(blockrow_gram_kernel<4>, 4); break;
        }
        HIPCHK(e);
        if (h->deterministic) {   // ... and the ordered sums of the pass's groups
            const dim3 rgrid((unsigned)(a.n_grp[0] + a.n_grp[1] + a.n_grp[2] + (pass == 0 ? 1 : 0)));
            const int32_t keys = h->gram_keys ? 1 : 0;
            switch (nb) {
                case 1: hipLaunchKernelGGL(blockrow_gram_reduce_kernel<1>, rgrid, dim3(256), 0, s, a, keys); break;
                case 2: hipLaunchKernelGGL(blockrow_gram_reduce_kernel<2>, rgrid, dim3(256), 0, s, a, keys); break;
                case 3: hipLaunchKernelGGL(blockrow_gram_reduce_kernel<3>, rgrid, dim3(256), 0, s, a, keys); break;
                default: hipLaunchKernelGGL(blockrow_gram_reduce_kernel<4>, rgrid, dim3(256), 0, s, a, keys); break;
            }
            HIPCHK(hipGetLastError());
        }
    }
    return PCS_OK;
}

int pcs_genchain_normal_blocks_device(pcs_genchain *h, const double *d_param_str, double *d_packed, void *stream) {
    if (!h || !d_param_str || !d_packed) return fail(PCS_ERR_ARG, "pcs_genchain_normal_blocks_device: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    return genchain_enqueue_normal(h, d_param_str, d_packed, stream ? (hipStream_t)stream : h->stream, nullptr);
}

// The prior of a generated chain: pcs_set_prior / pcs_get_prior / pcs_prior_add_device for this handle kind (the same store, the same kernels;
// the layout is genchain_layout, so a change of "dense_normal" is followed).
int pcs_genchain_set_prior(pcs_genchain *h, const double *mean, const double *inv_sigma, int64_t n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_set_prior: bad arguments");
    if (const int rc = PriorStore::check("pcs_genchain_set_prior", mean, inv_sigma, n, h->n_params)) return rc;
    if (!inv_sigma && h->prior.h_w.empty()) return PCS_OK;
    HIPCHK(hipSetDevice(h->device));
    if (h->prior.set_writes_device(inv_sigma)) HIPCHK(hipDeviceSynchronize());   // a trial's finish half that reads the old lists may be queued on any stream
    return h->prior.set(mean, inv_sigma, h->n_params);
}

int pcs_genchain_get_prior(pcs_genchain *h, double *mean, double *inv_sigma, int64_t capacity, int64_t *n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_get_prior: bad arguments");
    return h->prior.get("pcs_genchain_get_prior", mean, inv_sigma, capacity, n);
}

int pcs_genchain_prior_add_device(pcs_genchain *h, const double *d_param_str, double *d_packed, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_prior_add_device: bad arguments");
    return prior_add_piece("pcs_genchain_prior_add_device", h->device, h->prior, genchain_layout(h), h->n_params, d_param_str, d_packed, stream ? (hipStream_t)stream : h->stream);
}

// The box bounds of a generated chain: pcs_set_bounds / pcs_get_bounds / pcs_bounds_trials / pcs_bounds_active_device /
// pcs_bounds_truncate_device / pcs_lm_decide_bounded for this handle kind (the same store, the same kernels).
int pcs_genchain_set_bounds(pcs_genchain *h, const double *lo, const double *hi, int64_t n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_set_bounds: bad arguments");
    if (const int rc = BoundStore::check("pcs_genchain_set_bounds", lo, hi, n, h->n_params)) return rc;
    if (!lo && !h->bounds.active()) return PCS_OK;
    HIPCHK(hipSetDevice(h->device));
    if (h->bounds.set_writes_device(lo)) HIPCHK(hipDeviceSynchronize());   // a trial that reads the old lists may be queued on any stream
    return h->bounds.set(lo, hi, h->n_params);
}

int pcs_genchain_get_bounds(pcs_genchain *h, double *lo, double *hi, int64_t capacity, int64_t *n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_get_bounds: bad arguments");
    return h->bounds.get("pcs_genchain_get_bounds", lo, hi, capacity, n);
}

int pcs_genchain_bounds_trials(pcs_genchain *h, double *alpha_active, int64_t n_trials, int64_t *n_truncated) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_bounds_trials: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    return h->bounds.trials("pcs_genchain_bounds_trials", alpha_active, n_trials, n_truncated);
}

int pcs_genchain_bounds_active_device(pcs_genchain *h, const double *d_ps, const double *d_packed, const uint8_t *d_fixed, uint8_t *d_fixed_eff, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_bounds_active_device: bad arguments");
    return bounds_active_piece("pcs_genchain_bounds_active_device", h->device, h->bounds, genchain_layout(h), h->n_params, d_ps, d_packed, d_fixed, d_fixed_eff, stream ? (hipStream_t)stream : h->stream);
}

int pcs_genchain_bounds_truncate_device(pcs_genchain *h, const double *d_ps_in, double *d_delta, double *d_ps_out, double *d_alpha, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_bounds_truncate_device: bad arguments");
    return bounds_truncate_piece("pcs_genchain_bounds_truncate_device", h->device, h->bounds, h->n_params, d_ps_in, d_delta, d_ps_out, d_alpha, stream ? (hipStream_t)stream : h->stream);
}

int pcs_genchain_lm_decide_bounded(pcs_genchain *h, const double *d_cost_old, const double *d_cost_new, const double *d_dvec, const double *d_gm, const double *d_delta,
                                   const double *d_ps, const uint8_t *d_fixed_eff, const double *d_alpha, int32_t *d_status, double *d_lambda, double *d_stats, void *stream) {
    if (!h || !d_alpha) return fail(PCS_ERR_ARG, "pcs_genchain_lm_decide_bounded: bad arguments");
    if (!h->bounds.active()) return fail(PCS_ERR_STATE, "pcs_genchain_lm_decide_bounded: no bounds set");
    return lm_decide_piece("pcs_genchain_lm_decide_bounded", h->device, h->n_params, stream ? (hipStream_t)stream : h->stream, d_cost_old, d_cost_new, d_dvec, d_gm, d_delta, d_ps, d_fixed_eff, d_status, d_lambda, d_stats, d_alpha, h->bounds.pin());
}

// One Levenberg-Marquardt trial of a generated chain in two halves, like pcs_lm_trial_build / pcs_lm_trial_finish (same buffers, same
// shared build — pcs_solver.inc enqueue_lm_trial_build —, same decision kernel, same read-back).  The generated evaluation kernel reads its
// parameter string from a fixed address, so the trial is always built at ps[1] into packed[1] and an accepted one is copied over state 0:
// mode must hold PCS_LM_FIXED_TRIAL_BUFFER.
int pcs_genchain_lm_trial_build(pcs_genchain *h, const pcs_lm_buffers *b, void *stream) {
    const int rc = lm_check(h, b, "pcs_genchain_lm_trial_build");
    if (rc) return rc;
    if (!(b->mode & PCS_LM_FIXED_TRIAL_BUFFER)) return fail(PCS_ERR_ARG, "pcs_genchain_lm_trial_build: a generated chain builds its trial into packed[1] (mode PCS_LM_FIXED_TRIAL_BUFFER)");
    HIPCHK(hipSetDevice(h->device));
    LmTrialDesc d;
    d.who = "pcs_genchain_lm_trial_build"; d.device = h->device; d.n_cu = h->n_cu; d.n_params = h->n_params; d.L = genchain_layout(h);
    d.deterministic = h->deterministic; d.spd_timeout_us = h->spd_timeout_us;
    d.bounds = &h->bounds;
    d.fused = d.L.n_ent > 0 && d.L.n_lead > 0 && !h->bounds.active();   // with trailing entities always (without the slab preparation the completion does for the engines)
    d.finish_zeroes = true;   // (selector and empty_zero_state stay off: one state, and an empty table is refused by genchain_enqueue_normal with "no detections set")
    return enqueue_lm_trial_build(d, b, stream ? (hipStream_t)stream : h->stream,
                                  [&](hipStream_t s, bool) { return genchain_enqueue_normal(h, b->ps[1], b->packed[1], s, b->flags, true); });
}

// The pieces of a trial as calls of their own (pcs_solver.inc: schur_prepare_piece, schur_finish_piece, lm_decide_piece) for the handle's layout.
int pcs_genchain_schur_prepare(pcs_genchain *h, double *d_packed, const uint8_t *d_fixed, const double *d_lambda, double *d_linvt, double *d_u,
                               double *d_V, double *d_S, double *d_rhs, double *d_dvec, double *d_gm, int32_t *d_status, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_schur_prepare: bad arguments");
    return schur_prepare_piece("pcs_genchain_schur_prepare", h->device, genchain_layout(h), stream ? (hipStream_t)stream : h->stream, d_packed, d_fixed, d_lambda, d_linvt, d_u, d_V, d_S, d_rhs, d_dvec, d_gm, d_status);
}

int pcs_genchain_schur_finish(pcs_genchain *h, const double *d_linvt, const double *d_u, const double *d_w, const double *d_xlead, const uint8_t *d_fixed,
                              double *d_delta, const double *d_ps_in, double *d_ps_out, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_schur_finish: bad arguments");
    return schur_finish_piece("pcs_genchain_schur_finish", h->device, genchain_layout(h), stream ? (hipStream_t)stream : h->stream, d_linvt, d_u, d_w, d_xlead, d_fixed, d_delta, d_ps_in, d_ps_out);
}

int pcs_genchain_lm_decide(pcs_genchain *h, const double *d_cost_old, const double *d_cost_new, const double *d_dvec, const double *d_gm, const double *d_delta,
                           const double *d_ps, const uint8_t *d_fixed, int32_t *d_status, double *d_lambda, double *d_stats, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_lm_decide: bad arguments");
    return lm_decide_piece("pcs_genchain_lm_decide", h->device, h->n_params, stream ? (hipStream_t)stream : h->stream, d_cost_old, d_cost_new, d_dvec, d_gm, d_delta, d_ps, d_fixed, d_status, d_lambda, d_stats);
}

int pcs_genchain_lm_trial_finish(pcs_genchain *h, const pcs_lm_buffers *b, void *stream) {
    const int rc = lm_check(h, b, "pcs_genchain_lm_trial_finish");
    if (rc) return rc;
    if (!(b->mode & PCS_LM_FIXED_TRIAL_BUFFER)) return fail(PCS_ERR_ARG, "pcs_genchain_lm_trial_finish: mode must hold PCS_LM_FIXED_TRIAL_BUFFER");
    HIPCHK(hipSetDevice(h->device));
    return enqueue_lm_finish(h->n_cu, h->n_params, genchain_layout(h), h->prior, h->bounds, b, stream ? (hipStream_t)stream : h->stream);
}

int pcs_genchain_lm_trial(pcs_genchain *h, const pcs_lm_buffers *b, void *stream) {
    const int rc = pcs_genchain_lm_trial_build(h, b, stream);
    return rc ? rc : pcs_genchain_lm_trial_finish(h, b, stream);
}

int pcs_genchain_device_buffers(pcs_genchain *h, void **d_resid, void **d_jac) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_device_buffers: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    if (d_resid) *d_resid = h->d_resid.p;
    if (d_jac) *d_jac = h->d_jac.p;
    return PCS_OK;
}

int pcs_genchain_synchronize(pcs_genchain *h, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_synchronize: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(stream ? (hipStream_t)stream : h->stream));
    return PCS_OK;
}

int pcs_genchain_last_kernel_ms(pcs_genchain *h, float *slab_prep_ms, float *eval_ms) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_genchain_last_kernel_ms: bad arguments");
    if (!h->timed) return fail(PCS_ERR_STATE, "no evaluation has been queued yet");
    HIPCHK(hipEventSynchronize(h->ev[3]));
    float a = 0, b = 0;
    if (h->prep_timed) HIPCHK(hipEventElapsedTime(&a, h->ev[0], h->ev[1]));   // 0 for the one-launch form: there was no preparation launch
    HIPCHK(hipEventElapsedTime(&b, h->ev[2], h->ev[3]));
    if (slab_prep_ms) *slab_prep_ms = a;
    if (eval_ms) *eval_ms = b;
    return PCS_OK;
}

// The device Jacobian check of one user block (csrc/ba_blockcheck.hpp; abstract_function_block.test_self).  Synchronous; host buffers in
// and out; its own stream and buffers.  The code object states the shape it was built for (pcs_blockcheck_shape) and must agree.
int pcs_blockcheck(const char *code_object_path, int device, int np, int nin, int nout, int templated, const double *points, int64_t m,
                   double *fun_out, double *jac_out, double *fd_out) {
    if (!code_object_path || np < 1 || nin < 0 || nout < 1 || m < 1 || !points || !fun_out || !jac_out || !fd_out || (templated && nin != 0) ||
        np + nin > 64 || nout > 64 || m > ((int64_t)1 << 26))
        return fail(PCS_ERR_ARG, "pcs_blockcheck: bad arguments");
    if (const int rc = open_device("pcs_blockcheck", device, "the block check has no CPU fallback", true)) return rc;
    const int nrow = np + (templated ? 3 : nin), nc = np + nin;
    hipModule_t mod = nullptr;
    hipStream_t s = nullptr;
    DevBuf pts, outb;
    auto done = [&](int code) {
        if (s) (void)hipStreamSynchronize(s);
        pts.release(), outb.release();
        if (s) (void)hipStreamDestroy(s);
        if (mod) (void)hipModuleUnload(mod);
        return code;
    };
#define CHECK_CHK(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return done(fail(PCS_ERR_HIP, "%s failed: %s (pcs_blockcheck)", #expr, hipGetErrorString(_e))); \
    } while (0)
    CHECK_CHK(hipModuleLoad(&mod, code_object_path));
    hipDeviceptr_t d_shape = nullptr;
    size_t shape_bytes = 0;
    CHECK_CHK(hipModuleGetGlobal(&d_shape, &shape_bytes, mod, "pcs_blockcheck_shape"));
    int shape[4] = {};
    if (shape_bytes != sizeof(shape)) return done(fail(PCS_ERR_ARG, "pcs_blockcheck: the code object is not a block check"));
    CHECK_CHK(hipMemcpyDtoH(shape, d_shape, sizeof(shape)));
    if (shape[0] != np || shape[1] != nin || shape[2] != nout || shape[3] != (templated ? 1 : 0))
        return done(fail(PCS_ERR_ARG, "pcs_blockcheck: the code object checks a block of shape (np %d, nin %d, nout %d, templated %d), not (%d, %d, %d, %d)",
                         shape[0], shape[1], shape[2], shape[3], np, nin, nout, templated ? 1 : 0));
    hipFunction_t f = nullptr;
    CHECK_CHK(hipModuleGetFunction(&f, mod, "pcs_blockcheck"));
    CHECK_CHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    const size_t n_pts = (size_t)m * nrow, n_fun = (size_t)m * nout, n_jac = (size_t)m * nout * nc;
    CHECK_CHK(pts.alloc((int64_t)n_pts, sizeof(double)));
    CHECK_CHK(outb.alloc((int64_t)(n_fun + 2 * n_jac), sizeof(double)));
    double *d_pts = pts.as<double>(), *d_out = outb.as<double>();
    CHECK_CHK(hipMemcpyAsync(d_pts, points, sizeof(double) * n_pts, hipMemcpyHostToDevice, s));
    CHECK_CHK(hipMemsetAsync(d_out, 0, sizeof(double) * (n_fun + 2 * n_jac), s));
    BlockcheckArgs a{d_pts, m, d_out, d_out + n_fun, d_out + n_fun + n_jac};
    void *params[] = {&a};
    const int64_t threads = m * (nc + 1);
    CHECK_CHK(hipModuleLaunchKernel(f, (uint32_t)((threads + 255) / 256), 1, 1, 256, 1, 1, 0, s, params, nullptr));
    CHECK_CHK(hipMemcpyAsync(fun_out, d_out, sizeof(double) * n_fun, hipMemcpyDeviceToHost, s));
    CHECK_CHK(hipMemcpyAsync(jac_out, d_out + n_fun, sizeof(double) * n_jac, hipMemcpyDeviceToHost, s));
    CHECK_CHK(hipMemcpyAsync(fd_out, d_out + n_fun + n_jac, sizeof(double) * n_jac, hipMemcpyDeviceToHost, s));
    CHECK_CHK(hipStreamSynchronize(s));
#undef CHECK_CHK
    return done(PCS_OK);
}

}  // extern "C"
