// pcs_engine.hip — HIP kernels + C ABI of the MI355X bundle-adjustment cost/Jacobian engine.
//
// gfx950 (CDNA4) only: wave64, 256 CUs in 8 XCDs, 160 KiB LDS per CU, HBM3E.
// The path is an HBM-write-bound stream (380 B/detection for the FP64 template chain, of which
// 352 B are stores) with no dense contraction, so no MFMA there; the one contraction of the engine, the
// block-reduced normal equations, runs on the FP64 matrix cores (ba_normal.hpp).  See DESIGN.md.
//
// Kernels: ba_kernels.hpp (evaluation, compaction, legacy cost), ba_matfree.hpp (J products without J),
// ba_normal.hpp (J^T J / J^T r), ba_triangulate.hpp, ba_pnp.hpp, ba_pnp_consensus.hpp, ba_intrinsics.hpp, ba_intr_consensus.hpp, ba_riggraph.hpp, ba_twoview.hpp, ba_fivepoint.hpp, ba_align.hpp, ba_imagemap.hpp, ba_stereo.hpp, ba_stereo_sgm.hpp, ba_fusion.hpp, ba_sweep.hpp, ba_patchmatch.hpp; device maths: ba_device.hpp.  This file: the pcs_engine handle + its part of the C ABI; one translation unit with
// pcs_common.inc (errors, device queries), pcs_handle.inc (what every handle shares), pcs_dettable.inc (the detection table of both engine kinds), pcs_triangulator.inc, pcs_pnp.inc, pcs_intrinsics.inc, pcs_rig.inc, pcs_solver.inc (handle-free solver + the LM trial) and pcs_genchain.inc, included in that order.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <atomic>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/pcs_hip.h"
#include "ba_device.hpp"
#include "ba_kernels.hpp"
#include "ba_matfree.hpp"
#include "ba_normal.hpp"
#include "ba_reduce.hpp"
#include "ba_schur.hpp"
#include "ba_lm_fused.hpp"
#include "ba_prior.hpp"
#include "ba_bounds.hpp"
#include "ba_dense_chol.hpp"
#include "ba_chol_persist.hpp"
#include "ba_covariance.hpp"
#include "ba_triangulate.hpp"
#include "ba_tri_refine.hpp"
#include "ba_pnp.hpp"
#include "ba_consensus.hpp"
#include "ba_pnp_consensus.hpp"
#include "ba_tri_consensus.hpp"
#include "ba_rigpose.hpp"
#include "ba_intrinsics.hpp"
#include "ba_intr_consensus.hpp"
#include "ba_riggraph.hpp"
#include "ba_groupstats.hpp"
#include "ba_twoview.hpp"
#include "ba_fivepoint.hpp"
#include "ba_align.hpp"
#include "ba_imagemap.hpp"
#include "ba_stereo.hpp"
#include "ba_stereo_sgm.hpp"
#include "ba_fusion.hpp"
#include "ba_sweep.hpp"
#include "ba_patchmatch.hpp"
#include "ba_tsdf.hpp"
#include "ba_tsdf_raycast.hpp"
#include "ba_tsdf_colour.hpp"

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
using namespace pcs;

#include "pcs_common.inc"
#include "pcs_handle.inc"
#include "pcs_dettable.inc"
#include "pcs_triangulator.inc"
#include "pcs_pnp.inc"
#include "pcs_twoview.inc"
#include "pcs_align.inc"
#include "pcs_imagemap.inc"
#include "pcs_stereo.inc"
#include "pcs_fusion.inc"
#include "pcs_sweep.inc"
#include "pcs_patchmatch.inc"
#include "pcs_tsdf.inc"
#include "pcs_rigpose.inc"
#include "pcs_intrinsics.inc"
#include "pcs_rig.inc"
#include "pcs_stats.inc"
#include "pcs_solver.inc"

struct pcs_engine {
    int chain = 0, dtype = 0, device = 0, P = 0;
    int64_t n_cams = 0, n_imgs = 0, n_keys = 0, n_params = 0;
    int64_t extr_off = 0, pose_off = 0, point_off = 0;
    size_t msize = 8;   // bytes of a measurement scalar on the device (4 for PCS_F32); slabs and arithmetic are always FP64
    size_t osize = 8;   // bytes of the residual / Jacobian type written out (4 for PCS_F32 and PCS_MIXED)
    hipStream_t stream = nullptr;
    // ring of event quadruples: (slab_prep start, slab_prep stop, evaluation start, evaluation stop).  Both kernels carry their OWN
    // start / stop events (hipExtLaunchKernelGGL), so slab_prep's figure is its duration, not duration + the gap to the next
    // launch (round 2 reported start-to-start, 2.5 x what rocprofv3 sees); a one-launch step (PREP) has no slab_prep: 0.
    std::vector<hipEvent_t> ev;
    std::vector<uint8_t> ev_has_prep;   // per quadruple: a slab_prep launch was timed
    int64_t ev_ring = 1;         // quadruples in the ring
    int64_t ev_count = 0;        // evaluations recorded since the ring was (re)created
    bool events_valid = false;
    // Attach start/stop events to the kernel launches of every `timing_every`-th evaluation (0 = never).
    // Timed launches cost ~12 us of extra dispatch gaps per step on MI355X (profiles/r01/step_overhead.log),
    // so bench.py samples every 10th launch of its timed region instead of all of them.
    int64_t timing_every = 1;
    int64_t eval_count = 0;
    // Ordering across streams: `done` is recorded after everything the engine queues; the next piece of work that
    // touches the shared slabs / staging buffer / masks first waits for it — on the host where the host writes
    // (staging buffer, uploads), with hipStreamWaitEvent where another stream takes over.  (Round 1 kept a raw stream
    // handle and synchronised it later: a caller stream may be destroyed by then.)
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    bool have_done = false;
    bool done_pending = false;   // `done` still has to be recorded on done_stream (see flush_done)
    bool lazy_done = true;       // option "lazy_done_event" (A/B switch)
    bool lazy_any_stream = false;   // "lazy_done_event" = 2: also on caller streams (the caller keeps the stream alive until it resets the option)
    // static inputs
    DetStore det;                      // the detection table (pcs_dettable.inc); det.n = number of detections
    PriorStore prior;                  // the Gaussian parameter prior (pcs_set_prior); the handle's, not the table's
    BoundStore bounds;                 // the box bounds of the LM solve (pcs_set_bounds); the handle's, not the table's
    bool pack_indices = true;          // option "pack_indices" (A/B switch; takes effect at the next upload)
    DevBuf d_order;              // (cam, image)-sorted visiting order of a scattered table (normal equations), or empty
    DevBuf d_order_ck, d_order_ik;   // (cam, key) / (image, key) orders for the point passes
    // the detection table copied out in the visiting orders (index words; measurements except for the (image, key) pass): the
    // passes then stream their inputs instead of gathering 4 + 16 scattered bytes per detection through the order
    void *d_sorted[3][6] = {};   // per pass (shared — only for a scattered table —, (cam, key), (image, key)): packed, cam, img, key, uv, noise weights
    int sort_tables = 1;         // option: 0 = walk the original table through the visiting order (A/B)
    bool point_orders_tried = false;
    int normal_rows = 64;        // detections per LDS image of the normal-equations kernel (64 or 32)
    int waves_per_wg = 0;        // fused kernel: waves per workgroup (0 = automatic: fewer for small tables)
    bool have_template = false;
    // per-step
    DevBuf d_param;
    double *h_param = nullptr;  // pinned staging
    DevBuf d_cam_slab, d_pose_slab, d_points;
    DevBuf d_sink;  // 64 B: where tail lanes put their residual
    // scratch outputs for the host-buffer entry points
    DevBuf d_resid, d_jac;
    // compaction
    DevBuf d_keep, d_row_off;   // uint32 masks, int64 offsets
    int64_t nnz = -1;
    DevBuf d_data;
    // matrix-free operators (f2)
    DevBuf d_vin, d_vout, d_cost;
    // normal equations (f2): scratch of the host-buffer entry point
    DevBuf d_H;
    // legacy cost (f3)
    DevBuf d_im_points, d_cam_tab;
    bool linearized = false;
    int normal_debug = 0;
    int normal_imgkey_wgs_per_cu = 0;   // 0 = default (48)
    int normal_imgkey_product = 1;   // pose-point blocks by ba_normal_imgkey_kernel (0: the boundary-walking pass, kept for A/B)
    bool matfree_lds = true;  // accumulate J^T products in workgroup-private LDS before the global atomics
    // launch geometry
    int n_cu = 256;
    // Launch geometry.  variant < 0 / wgs_per_cu <= 0 = automatic, from the MI355X sweeps in
    // profiles/r01/sweeps.md: transposed + non-temporal stores always; for a table whose 64-detection
    // tiles are (cam, image)-uniform (the reference's cam -> image -> key order) slabs are read
    // through L1/L2 with many small workgroups; for scattered tables slabs are staged in LDS by
    // few long-lived workgroups.
    int variant = -1;
    int64_t wgs_per_cu = 0;
    int compact_variant = 1;     // 1 = tile kernel with coalesced stores, 0 = per-lane stores
    bool xcd_remap = false;      // contiguous eighth of the table per XCD group (experiment; no measured effect)
    double tile_locality = 1.0;  // fraction of 64-detection tiles touching <= 2 distinct (cam, image) pairs
    double tile_segments = 1.0;  // mean number of (cam, image) runs per 64-detection tile (1.0 = every tile inside one run)
    // One-launch step: the evaluation kernel prepares the slabs of its tile per wave instead of a slab_prep launch in front
    // (ba_eval_kernel<..., PREP>).  -1 = automatic: run-ordered tables (few (camera, image) runs per tile); FP64 outputs at
    // any size (measured on MI355X, profiles/r03: rig-32 71.2 -> 65.0 us per step, rig-32-self 82.0 -> 78.7, free 60.1 -> 57.4,
    // an 8-way shard 14.2 -> 12.3, ring-8 12.3 -> 10.3), float outputs and residual-only evaluations only up to
    // fuse_prep_max_n detections (those kernels are issue-bound at large N: rig-32 mixed 35.3 -> 53.4 us, rig-128 f32 294 -> 500 us,
    // residual only at N = 1e6 9 + 4.4 -> 24.6 us with it).
    int fuse_prep = -1;
    int64_t fuse_prep_max_n = 250000;
    int64_t tiles_per_wg = 0;  // 0 = derive from wgs_per_cu
    size_t lds_limit = 160 * 1024;
    // time limit of every wait inside the one-launch dense solve of an LM trial (csrc/ba_chol_persist.hpp); option "spd_timeout_us"
    int64_t spd_timeout_us = 250000;
    // option "deterministic": every sum of the normal equations and of the Schur step is taken in an order the table and the launch
    // geometry fix (csrc/ba_reduce.hpp) instead of with f64 atomics in arrival order: two runs — and the ranks of a sharded loop — compute
    // the same bits
    int deterministic = 0;
    // pcs_set_loss: robust loss of every normal-equation build (ba_device.hpp robust_rho; 0 = linear) and its f_scale
    int loss = 0;
    double f_scale = 1.0;
    int fused_trial = 1;   // option: pcs_lm_trial_build uses schur_prep_kernel / schur_finish_kernel (csrc/ba_lm_fused.hpp); 0 = the separate launches (A/B)
    // host copies of the visiting orders (shared pass of a scattered table, (cam, key) pass): the deterministic mode's tables are built from them
    std::vector<int32_t> h_order, h_order_ck;
    // static tables + workspaces of the ordered second pass, per MFMA pass (0 shared, 1 (cam, key)); built at the first deterministic
    // build for the launch geometry in use, rebuilt when the table or the geometry changes
    struct DetPass {
        int64_t n = -1;
        int64_t tpw = 0;
        int32_t n_seg = 0, n_lr = 0, n_grp = 0, n_ent = 0, n_waves = 0;
        int32_t *d_idx = nullptr;      // one allocation: seg_base | lr_ptr | lr_segs | lr_ka | lr_kb | grp_ptr | cam_ptr | ent_ptr | ent_runs
        int64_t off[9] = {};
        double *d_work = nullptr;      // one allocation: part | Q | G | wave_cost (n_waves: the robust loss's cost, shared pass)
        int64_t work_off[4] = {};
    } det_pass[2];
};

// `done` is recorded LAZILY where that is safe (round 3): an event record is a packet of its own between two launches, and a
// small step (config 2, an 8-way shard) paid for one after every evaluation although nothing ever waited for it.  For work
// queued on the engine's own stream or on the default stream (handles that outlive every call) mark_done only notes the
// stream; the record happens when somebody needs to wait — it then covers everything queued on that stream so far, a
// superset.  Work on any other caller stream is recorded at once: that stream may be destroyed before the next call.
// (The batched handles record after every run: RunFence in pcs_handle.inc.)
static hipError_t flush_done(pcs_engine *h) {
    if (!h->done_pending) return hipSuccess;
    h->done_pending = false;
    return hipEventRecord(h->done, h->done_stream);
}
// everything queued so far has finished (host-side wait)
static hipError_t wait_done_host(pcs_engine *h) {
    if (!h->have_done) return hipSuccess;
    hipError_t e = flush_done(h);
    return e != hipSuccess ? e : hipEventSynchronize(h->done);
}
// work queued on `s` from here on runs after everything queued so far, whatever stream that was on.  Same stream as the
// previous enqueue: stream order already gives that.  Another stream: a device-side wait — except for the legacy
// default-stream handle, on which hipStreamWaitEvent of this runtime faults; the (rare) switch to or from it waits on the host.
static hipError_t order_after_done(pcs_engine *h, hipStream_t s) {
    if (!h->have_done || s == h->done_stream) return hipSuccess;
    hipError_t e = flush_done(h);
    if (e != hipSuccess) return e;
    if (s == hipStreamLegacy || s == nullptr || h->done_stream == hipStreamLegacy) return hipEventSynchronize(h->done);
    return hipStreamWaitEvent(s, h->done, 0);
}
static hipError_t mark_done(pcs_engine *h, hipStream_t s) {
    // (every enqueue calls order_after_done(h, s) first, so work on an earlier stream is already ordered before `s`)
    h->have_done = true;
    h->done_stream = s;   // used as a handle again only when it is the engine's own stream or the default stream
    if (h->lazy_done && (h->lazy_any_stream || s == h->stream || s == hipStreamLegacy)) {
        h->done_pending = true;
        return hipSuccess;
    }
    h->done_pending = false;
    return hipEventRecord(h->done, s);
}

// the event quadruple the next timed piece of work records into (see pcs_engine::ev)
static hipEvent_t *ring_slot(pcs_engine *h, bool has_prep) {
    const int64_t i = h->ev_count % h->ev_ring;
    h->ev_has_prep[i] = has_prep ? 1 : 0;
    return h->ev.data() + 4 * i;
}
// (slab_prep ms — 0 when that quadruple timed no slab_prep launch —, evaluation ms) of quadruple i; waits for it
static int ring_read(pcs_engine *h, int64_t i, float *prep_ms, float *eval_ms) {
    hipEvent_t *ev = h->ev.data() + 4 * i;
    HIPCHK(hipEventSynchronize(ev[3]));
    *prep_ms = 0.f;
    if (h->ev_has_prep[i]) HIPCHK(hipEventElapsedTime(prep_ms, ev[0], ev[1]));
    HIPCHK(hipEventElapsedTime(eval_ms, ev[2], ev[3]));
    return PCS_OK;
}

static int64_t padded_points(int64_t n_keys) { return (n_keys * 3 + 3) & ~(int64_t)3; }

static void free_det_tables(pcs_engine *h) {
    for (auto &d : h->det_pass) {
        if (d.d_idx) (void)hipFree(d.d_idx);
        if (d.d_work) (void)hipFree(d.d_work);
        d = pcs_engine::DetPass{};
    }
}

static void free_sorted_tables(pcs_engine *h) {
    for (auto &t : h->d_sorted)
        for (void *&b : t) {
            if (b) (void)hipFree(b);
            b = nullptr;
        }
}

// the passes' sorted copies of the noise weights (pcs_set_weights replaces the weights, not the table); the caller has waited
static void free_sorted_weights(pcs_engine *h) {
    for (auto &t : h->d_sorted) {
        if (t[5]) (void)hipFree(t[5]);
        t[5] = nullptr;
    }
}

// everything a new detection table replaces (a smaller table gives its memory back); the caller has waited for the work that reads it
static void release_table(pcs_engine *h) {
    h->det.release();
    for (DevBuf *b : {&h->d_order, &h->d_order_ck, &h->d_order_ik, &h->d_resid, &h->d_jac, &h->d_keep, &h->d_row_off, &h->d_data}) b->release();
    free_sorted_tables(h);
    free_det_tables(h);
    h->point_orders_tried = false;
    h->nnz = -1;
    h->h_order.clear();
    h->h_order_ck.clear();
}

extern "C" {

int pcs_create(pcs_engine **out, int chain, int dtype, int64_t n_cams, int64_t n_imgs, int64_t n_keys, int device) {
    if (!out) return fail(PCS_ERR_ARG, "pcs_create: out is NULL");
    *out = nullptr;
    if (chain < 0 || chain > 2) return fail(PCS_ERR_ARG, "pcs_create: chain %d not in {0,1,2}", chain);
    if (dtype != PCS_F64 && dtype != PCS_F32 && dtype != PCS_MIXED) return fail(PCS_ERR_ARG, "pcs_create: dtype %d not in {0,1,2}", dtype);
    if (n_cams <= 0 || n_keys <= 0 || (chain != PCS_CHAIN_FREE && n_imgs <= 0))
        return fail(PCS_ERR_ARG, "pcs_create: counts must be positive (cams %lld imgs %lld keys %lld)", (long long)n_cams,
                    (long long)n_imgs, (long long)n_keys);
    if (n_cams > (1 << 24) || n_imgs > (1 << 24) || n_keys > (1 << 26)) return fail(PCS_ERR_ARG, "pcs_create: counts too large");
    if (const int rc = open_device("pcs_create", device, "this engine has no CPU fallback", true)) return rc;
    pcs_engine *h = new pcs_engine();
    h->chain = chain;
    h->dtype = dtype;
    h->device = device;
    h->P = chain_P(chain);
    h->msize = dtype == PCS_F32 ? 4 : 8;
    h->osize = dtype == PCS_F64 ? 8 : 4;
    h->n_cams = n_cams;
    h->n_imgs = chain == PCS_CHAIN_FREE ? 0 : n_imgs;
    h->n_keys = n_keys;
    h->extr_off = 9 * n_cams;
    h->pose_off = 15 * n_cams;
    h->point_off = chain == PCS_CHAIN_SELF ? 15 * n_cams + 6 * n_imgs : 15 * n_cams;
    h->n_params = chain == PCS_CHAIN_TEMPLATE ? 15 * n_cams + 6 * n_imgs
                  : chain == PCS_CHAIN_SELF   ? 15 * n_cams + 6 * n_imgs + 3 * n_keys
                                              : 15 * n_cams + 3 * n_keys;
    h->ev.assign(4, nullptr);
    h->ev_has_prep.assign(1, 0);
    // the steps of the set-up in order; the first that fails is named in the error and ends it
    hipError_t e = hipSuccess;
    const char *failed = nullptr;
    auto step = [&](const char *what, hipError_t r) {
        if (r != hipSuccess) e = r, failed = what;
        return r == hipSuccess;
    };
    hipDeviceProp_t prop;
    bool ok = step("hipGetDeviceProperties", hipGetDeviceProperties(&prop, device));
    if (ok) {
        h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        h->lds_limit = prop.maxSharedMemoryPerMultiProcessor > 0 ? prop.maxSharedMemoryPerMultiProcessor
                       : prop.sharedMemPerBlock > 0            ? prop.sharedMemPerBlock
                                                               : 64 * 1024;
        ok = step("hipStreamCreateWithFlags", hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    }
    for (auto &ev : h->ev) ok = ok && step("hipEventCreate", hipEventCreate(&ev));
    ok = ok && step("hipEventCreateWithFlags(done)", hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
    ok = ok && step("hipHostMalloc(h_param)", hipHostMalloc(reinterpret_cast<void **>(&h->h_param), sizeof(double) * h->n_params, hipHostMallocDefault));
    struct { const char *what; DevBuf &b; int64_t n; } fixed[] = {{"hipMalloc(d_param)", h->d_param, h->n_params}, {"hipMalloc(d_cam_slab)", h->d_cam_slab, n_cams * CAM_STRIDE},
                                                                  {"hipMalloc(d_pose_slab)", h->d_pose_slab, std::max<int64_t>(1, h->n_imgs) * POSE_STRIDE},
                                                                  {"hipMalloc(d_points)", h->d_points, padded_points(n_keys)}, {"hipMalloc(d_sink)", h->d_sink, 8}};
    for (auto &f : fixed) ok = ok && step(f.what, f.b.alloc(f.n, sizeof(double)));
    ok = ok && step("hipMemset(d_points)", hipMemset(h->d_points.p, 0, sizeof(double) * padded_points(n_keys)));
    if (!ok) {
        const int rc = fail(PCS_ERR_HIP, "%s failed: %s (pcs_create)", failed, hipGetErrorString(e));
        pcs_destroy(h);   // releases whatever was allocated so far
        return rc;
    }
    *out = h;
    return PCS_OK;
}

int pcs_destroy(pcs_engine *h) {
    if (!h) return PCS_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    release_table(h);   // what belongs to the detection table; then the buffers that outlive a table
    h->prior.release();
    h->bounds.release();
    for (DevBuf *b : {&h->d_param, &h->d_cam_slab, &h->d_pose_slab, &h->d_points, &h->d_sink, &h->d_vin, &h->d_vout, &h->d_cost, &h->d_H, &h->d_im_points, &h->d_cam_tab})
        b->release();
    if (h->h_param) (void)hipHostFree(h->h_param);
    for (auto &e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->done) (void)hipEventDestroy(h->done);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return PCS_OK;
}

int64_t pcs_n_params(const pcs_engine *h) { return h ? h->n_params : -1; }
int pcs_row_len(const pcs_engine *h) { return h ? h->P : -1; }
int64_t pcs_n_detections(const pcs_engine *h) { return h ? h->det.n : -1; }

static DetCounts det_counts(const pcs_engine *h) { return DetCounts{h->n_cams, h->n_imgs, h->n_keys, h->chain == PCS_CHAIN_FREE}; }

static int upload_detections(pcs_engine *h, DetColumns &c, const double *uv) {
    // the engine's own tables are only replaced once the new ones are known to be good
    const DetCounts counts = det_counts(h);
    if (const int rc = det_check_range(c, counts)) return rc;
    const int64_t n = (int64_t)c.cam.size();
    double locality = 1.0, segments = 1.0;
    {   // slab-read locality of the table, per 64-detection tile (drives the automatic variant choice)
        int64_t tiles = 0, good = 0, runs = 0;
        for (int64_t t0 = 0; t0 < n; t0 += TILE, ++tiles) {
            const int64_t t1 = std::min<int64_t>(t0 + TILE, n);
            int64_t p0 = -1, p1 = -1, prev = -1;
            bool ok = true;
            for (int64_t i = t0; i < t1; ++i) {
                const int64_t pr = ((int64_t)c.cam[i] << 32) | (counts.no_img ? 0u : (uint32_t)c.img[i]);
                runs += pr != prev;   // an upper bound of the distinct pairs of the tile; exact for run-ordered tables
                prev = pr;
                if (pr == p0 || pr == p1) continue;
                if (p0 < 0) p0 = pr; else if (p1 < 0) p1 = pr; else ok = false;
            }
            good += ok;
        }
        if (tiles) locality = (double)good / (double)tiles, segments = (double)runs / (double)tiles;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(wait_done_host(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    release_table(h);   // det.n stays 0 (= "no detections set") if an allocation or copy below fails
    h->tile_locality = locality;
    h->tile_segments = segments;
    if (n > 0 && locality < 0.5 && n <= INT32_MAX) {
        // scattered table: a (cam, image)-sorted visiting order for the kernels whose result does not depend on
        // the row order (ba_normal_kernel keeps its accumulators per (cam, image) run)
        std::vector<int32_t> order(n);
        for (int64_t i = 0; i < n; ++i) order[i] = (int32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return c.cam[x] != c.cam[y] ? c.cam[x] < c.cam[y] : c.img[x] < c.img[y]; });
        if (const int rc = h->d_order.grow(n, sizeof(int32_t))) return rc;
        HIPCHK(hipMemcpy(h->d_order.p, order.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
        h->h_order.swap(order);
    }
    return h->det.upload(c, uv, counts, h->pack_indices, h->msize == 4);
}

int pcs_set_detections_table(pcs_engine *h, const double *det5, int64_t n) {
    if (!h || (!det5 && n > 0) || n < 0) return fail(PCS_ERR_ARG, "pcs_set_detections_table: bad arguments");
    DetColumns c;
    std::vector<double> uv;
    if (const int rc = det_parse(det5, n, c, uv)) return rc;
    return upload_detections(h, c, uv.data());
}

int pcs_set_detections(pcs_engine *h, const int32_t *cam, const int32_t *img, const int32_t *key, const double *uv, int64_t n) {
    if (!h || n < 0 || (n > 0 && (!cam || !key || !uv || (!img && h->chain != PCS_CHAIN_FREE))))
        return fail(PCS_ERR_ARG, "pcs_set_detections: bad arguments");
    DetColumns c;
    c.cam.assign(cam, cam + n), c.key.assign(key, key + n);
    if (img) c.img.assign(img, img + n); else c.img.assign(n, 0);
    return upload_detections(h, c, uv);
}

int pcs_set_template(pcs_engine *h, const double *points) {
    if (!h || !points) return fail(PCS_ERR_ARG, "pcs_set_template: bad arguments");
    if (h->chain != PCS_CHAIN_TEMPLATE) return fail(PCS_ERR_ARG, "pcs_set_template: only the template chain has constant points");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(wait_done_host(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(h->d_points.p, points, sizeof(double) * 3 * h->n_keys, hipMemcpyHostToDevice));
    h->have_template = true;
    return PCS_OK;
}

int pcs_set_option(pcs_engine *h, const char *key, int64_t value) {
    if (!h || !key) return fail(PCS_ERR_ARG, "pcs_set_option: bad arguments");
    if (!strcmp(key, "variant")) {
        if (value < -1 || value > 7) return fail(PCS_ERR_ARG, "variant must be in [-1,7] (-1 = automatic)");
        h->variant = (int)value;
    } else if (!strcmp(key, "wgs_per_cu")) {
        if (value < 0 || value > 64) return fail(PCS_ERR_ARG, "wgs_per_cu must be in [0,64] (0 = automatic)");
        h->wgs_per_cu = value;
        h->tiles_per_wg = 0;
    } else if (!strcmp(key, "timing_every")) {
        if (value < 0 || value > 1000000) return fail(PCS_ERR_ARG, "timing_every must be in [0,1000000]");
        h->timing_every = value;
        h->eval_count = 0;
    } else if (!strcmp(key, "fuse_prep")) {
        if (value < -1 || value > 1) return fail(PCS_ERR_ARG, "fuse_prep must be -1 (automatic), 0 (slab_prep launch) or 1 (waves prepare their slabs)");
        h->fuse_prep = (int)value;
    } else if (!strcmp(key, "fuse_prep_max_n")) {
        if (value < 0) return fail(PCS_ERR_ARG, "fuse_prep_max_n must be >= 0");
        h->fuse_prep_max_n = value;
    } else if (!strcmp(key, "lazy_done_event")) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(flush_done(h));
        if (value < 0 || value > 2) return fail(PCS_ERR_ARG, "lazy_done_event must be 0, 1 or 2");
        h->lazy_done = value != 0;
        h->lazy_any_stream = value == 2;
    } else if (!strcmp(key, "xcd_remap")) {
        h->xcd_remap = value != 0;
    } else if (!strcmp(key, "waves_per_wg")) {
        if (value < 0 || value > WAVES_PER_WG || value == 3) return fail(PCS_ERR_ARG, "waves_per_wg must be 0 (automatic), 1, 2 or 4");
        h->waves_per_wg = (int)value;
    } else if (!strcmp(key, "pack_indices")) {
        h->pack_indices = value != 0;   // takes effect at the next pcs_set_detections*
    } else if (!strcmp(key, "normal_rows")) {
        if (value != 32 && value != 64) return fail(PCS_ERR_ARG, "normal_rows must be 32 or 64");
        h->normal_rows = (int)value;
    } else if (!strcmp(key, "matfree_lds")) {
        h->matfree_lds = value != 0;
    } else if (!strcmp(key, "normal_debug")) {
        h->normal_debug = (int)value;
    } else if (!strcmp(key, "normal_sort_tables")) {
        h->sort_tables = value != 0;
    } else if (!strcmp(key, "normal_imgkey_product")) {
        h->normal_imgkey_product = value != 0;
    } else if (!strcmp(key, "normal_imgkey_wgs_per_cu")) {
        h->normal_imgkey_wgs_per_cu = (int)value;
    } else if (!strcmp(key, "compact_variant")) {
        if (value < 0 || value > 1) return fail(PCS_ERR_ARG, "compact_variant must be 0 or 1");
        h->compact_variant = (int)value;
    } else if (!strcmp(key, "event_ring")) {
        // keep the HIP-event triples of the last `value` evaluations (pcs_kernel_ms_mean averages them)
        if (value < 1 || value > 100000) return fail(PCS_ERR_ARG, "event_ring must be in [1,100000]");
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(wait_done_host(h));
        for (auto &e : h->ev)
            if (e) (void)hipEventDestroy(e);
        h->ev.assign(4 * value, nullptr);
        h->ev_has_prep.assign(value, 0);
        for (auto &e : h->ev) HIPCHK(hipEventCreate(&e));
        h->ev_ring = value;
        h->ev_count = 0;
        h->events_valid = false;
    } else if (!strcmp(key, "fused_trial")) {
        h->fused_trial = value != 0;
    } else if (!strcmp(key, "deterministic")) {
        if (value < 0 || value > 1) return fail(PCS_ERR_ARG, "deterministic must be 0 or 1");
        h->deterministic = (int)value;
    } else if (!strcmp(key, "spd_timeout_us")) {
        // how long a workgroup of the one-launch dense solve waits for a hand-over before it abandons the launch (status bit 2, LM stop
        // code 9: the trial is repeated with the launch-per-column form).  Tests set it to 1 us to force that path.
        if (value < 1 || value > 60000000) return fail(PCS_ERR_ARG, "spd_timeout_us must be in [1, 60000000]");
        h->spd_timeout_us = value;
    } else if (!strcmp(key, "tiles_per_wg")) {
        if (value < 0 || value > (1 << 20)) return fail(PCS_ERR_ARG, "tiles_per_wg out of range");
        h->tiles_per_wg = value;
    } else {
        return fail(PCS_ERR_ARG, "pcs_set_option: unknown key '%s'", key);
    }
    return PCS_OK;
}

static_assert(PCS_LOSS_LINEAR == LOSS_LINEAR && PCS_LOSS_HUBER == LOSS_HUBER && PCS_LOSS_SOFT_L1 == LOSS_SOFT_L1 && PCS_LOSS_CAUCHY == LOSS_CAUCHY &&
              PCS_LOSS_ARCTAN == LOSS_ARCTAN, "loss kinds of the C ABI and of ba_device.hpp");
int pcs_set_loss(pcs_engine *h, int kind, double f_scale) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_set_loss: bad arguments");
    if (kind < PCS_LOSS_LINEAR || kind > PCS_LOSS_ARCTAN) return fail(PCS_ERR_ARG, "pcs_set_loss: kind %d not in [0, 4] (linear, huber, soft_l1, cauchy, arctan)", kind);
    if (!std::isfinite(f_scale) || !(f_scale > 0.0)) return fail(PCS_ERR_ARG, "pcs_set_loss: f_scale must be finite and > 0 (got %g)", f_scale);
    h->loss = kind;
    h->f_scale = f_scale;
    return PCS_OK;
}

int pcs_get_loss(pcs_engine *h, int *kind, double *f_scale) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_get_loss: bad arguments");
    if (kind) *kind = h->loss;
    if (f_scale) *f_scale = h->f_scale;
    return PCS_OK;
}

int pcs_set_weights(pcs_engine *h, const double *inv_sigma, int64_t n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_set_weights: bad arguments");
    if (inv_sigma) {   // everything is checked before anything changes: a refused call leaves the previous weights in force
        if (n != h->det.n) return fail(PCS_ERR_ARG, "pcs_set_weights: %lld weights for a table of %lld detections", (long long)n, (long long)h->det.n);
        for (int64_t i = 0; i < n; ++i)
            if (!std::isfinite(inv_sigma[i]) || !(inv_sigma[i] > 0.0))
                return fail(PCS_ERR_ARG, "pcs_set_weights: weight %lld = %g must be finite and > 0", (long long)i, inv_sigma[i]);
    }
    if (!inv_sigma && !h->det.w.p) return PCS_OK;   // nothing set, nothing to clear: no device call
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(wait_done_host(h));   // a build that reads the old weights (or their sorted copies) may still run
    HIPCHK(hipStreamSynchronize(h->stream));
    free_sorted_weights(h);
    return h->det.set_weights(inv_sigma);
}

int pcs_get_weights(pcs_engine *h, double *inv_sigma, int64_t capacity, int64_t *n) {
    if (!h || capacity < 0 || (!inv_sigma && !n)) return fail(PCS_ERR_ARG, "pcs_get_weights: bad arguments");
    const int64_t have = h->det.w.p ? h->det.n : 0;
    if (n) *n = have;
    const int64_t m = std::min(have, capacity);
    if (inv_sigma && m > 0) {
        HIPCHK(hipSetDevice(h->device));
        HIPCHK(hipMemcpy(inv_sigma, h->det.w.p, sizeof(double) * m, hipMemcpyDeviceToHost));
    }
    return PCS_OK;
}

int pcs_set_prior(pcs_engine *h, const double *mean, const double *inv_sigma, int64_t n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_set_prior: bad arguments");
    if (const int rc = PriorStore::check("pcs_set_prior", mean, inv_sigma, n, h->n_params)) return rc;
    if (!inv_sigma && h->prior.h_w.empty()) return PCS_OK;   // nothing set, nothing to clear: no device call
    HIPCHK(hipSetDevice(h->device));
    if (h->prior.set_writes_device(inv_sigma)) {   // a trial's finish half that reads the old lists may be queued on any stream
        HIPCHK(wait_done_host(h));
        HIPCHK(hipDeviceSynchronize());
    }
    return h->prior.set(mean, inv_sigma, h->n_params);
}

int pcs_get_prior(pcs_engine *h, double *mean, double *inv_sigma, int64_t capacity, int64_t *n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_get_prior: bad arguments");
    return h->prior.get("pcs_get_prior", mean, inv_sigma, capacity, n);
}

int pcs_set_bounds(pcs_engine *h, const double *lo, const double *hi, int64_t n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_set_bounds: bad arguments");
    if (const int rc = BoundStore::check("pcs_set_bounds", lo, hi, n, h->n_params)) return rc;
    if (!lo && !h->bounds.active()) return PCS_OK;   // nothing set, nothing to clear: no device call
    HIPCHK(hipSetDevice(h->device));
    if (h->bounds.set_writes_device(lo)) {   // a trial that reads the old lists may be queued on any stream
        HIPCHK(wait_done_host(h));
        HIPCHK(hipDeviceSynchronize());
    }
    return h->bounds.set(lo, hi, h->n_params);
}

int pcs_get_bounds(pcs_engine *h, double *lo, double *hi, int64_t capacity, int64_t *n) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_get_bounds: bad arguments");
    return h->bounds.get("pcs_get_bounds", lo, hi, capacity, n);
}

int pcs_bounds_trials(pcs_engine *h, double *alpha_active, int64_t n_trials, int64_t *n_truncated) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_bounds_trials: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    return h->bounds.trials("pcs_bounds_trials", alpha_active, n_trials, n_truncated);
}

}  // extern "C"

// ---- launch plumbing ---------------------------------------------------------------------------
// Kernel timing uses the start/stop events of hipExtLaunchKernelGGL: the timestamps are taken by the
// dispatch itself, without the extra barrier packets that hipEventRecord would put between kernels.
struct EvPair { hipEvent_t start, stop; };

template <int CHAIN, int MODE, int VARIANT, typename TO, bool PREP = false>
static hipError_t launch_eval_v(const EvalArgs &a, dim3 grid, int threads, size_t lds, hipStream_t s, EvPair ev) {
    auto kern = ba_eval_kernel<CHAIN, MODE, VARIANT, TO, PREP>;
    // per device: largest dynamic-LDS size already enabled for this kernel.  Handles driven from different host threads
    // may get here together: the value is monotone and setting the attribute twice is harmless, so an atomic max is enough
    static std::atomic<size_t> configured[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::atomic<size_t> &cfg = configured[dev & 63];
    if (lds > 48 * 1024 && lds > cfg.load(std::memory_order_acquire)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        size_t seen = cfg.load(std::memory_order_relaxed);
        while (seen < lds && !cfg.compare_exchange_weak(seen, lds, std::memory_order_release, std::memory_order_relaxed)) {}
    }
    hipExtLaunchKernelGGL(kern, grid, dim3(threads), (std::uint32_t)lds, s, ev.start, ev.stop, 0, a);
    return hipGetLastError();
}

template <int CHAIN, int MODE, typename TO>
static hipError_t launch_eval_m(int variant, bool prep, const EvalArgs &a, dim3 grid, int threads, size_t lds, hipStream_t s, EvPair ev) {
    if (prep) {   // one-launch step: slabs through L1/L2 is the only form it replaces; transposed stores whenever there is a Jacobian
        if constexpr (MODE == MODE_RESID) {
            return (variant & VAR_NT) ? launch_eval_v<CHAIN, MODE, VAR_NT, TO, true>(a, grid, threads, lds, s, ev)
                                      : launch_eval_v<CHAIN, MODE, 0, TO, true>(a, grid, threads, lds, s, ev);
        } else {
            return (variant & VAR_NT) ? launch_eval_v<CHAIN, MODE, VAR_TRANSPOSE | VAR_NT, TO, true>(a, grid, threads, lds, s, ev)
                                      : launch_eval_v<CHAIN, MODE, VAR_TRANSPOSE, TO, true>(a, grid, threads, lds, s, ev);
        }
    }
    switch (variant) {
        case 0: return launch_eval_v<CHAIN, MODE, 0, TO>(a, grid, threads, lds, s, ev);
        case 1: return launch_eval_v<CHAIN, MODE, 1, TO>(a, grid, threads, lds, s, ev);
        case 2: return launch_eval_v<CHAIN, MODE, 2, TO>(a, grid, threads, lds, s, ev);
        case 3: return launch_eval_v<CHAIN, MODE, 3, TO>(a, grid, threads, lds, s, ev);
        case 4: return launch_eval_v<CHAIN, MODE, 4, TO>(a, grid, threads, lds, s, ev);
        case 5: return launch_eval_v<CHAIN, MODE, 5, TO>(a, grid, threads, lds, s, ev);
        case 6: return launch_eval_v<CHAIN, MODE, 6, TO>(a, grid, threads, lds, s, ev);
        default: return launch_eval_v<CHAIN, MODE, 7, TO>(a, grid, threads, lds, s, ev);
    }
}

template <int CHAIN, typename TO>
static hipError_t launch_eval_c(int mode, int variant, bool prep, const EvalArgs &a, dim3 grid, int threads, size_t lds, hipStream_t s, EvPair ev) {
    switch (mode) {
        case MODE_RESID: return launch_eval_m<CHAIN, MODE_RESID, TO>(variant & ~VAR_TRANSPOSE, prep, a, grid, threads, lds, s, ev);
        case MODE_JAC: return launch_eval_m<CHAIN, MODE_JAC, TO>(variant, prep, a, grid, threads, lds, s, ev);
        default: return launch_eval_m<CHAIN, MODE_RESID | MODE_JAC, TO>(variant, prep, a, grid, threads, lds, s, ev);
    }
}

template <typename TO>
static hipError_t launch_eval_t(int chain, int mode, int variant, bool prep, const EvalArgs &a, dim3 grid, int threads, size_t lds, hipStream_t s, EvPair ev) {
    switch (chain) {
        case CHAIN_TEMPLATE: return launch_eval_c<CHAIN_TEMPLATE, TO>(mode, variant, prep, a, grid, threads, lds, s, ev);
        case CHAIN_SELF: return launch_eval_c<CHAIN_SELF, TO>(mode, variant, prep, a, grid, threads, lds, s, ev);
        default: return launch_eval_c<CHAIN_FREE, TO>(mode, variant, prep, a, grid, threads, lds, s, ev);
    }
}

template <int CHAIN, typename TO>
static hipError_t launch_compact_tile_c(int mode, const EvalArgs &a, dim3 grid, size_t lds, hipStream_t s) {
    if (mode == MODE_RESID) hipLaunchKernelGGL((ba_compact_tile_kernel<CHAIN, MODE_RESID, TO>), grid, dim3(WG_THREADS), lds, s, a);
    else if (mode == MODE_JAC) hipLaunchKernelGGL((ba_compact_tile_kernel<CHAIN, MODE_JAC, TO>), grid, dim3(WG_THREADS), lds, s, a);
    else hipLaunchKernelGGL((ba_compact_tile_kernel<CHAIN, MODE_RESID | MODE_JAC, TO>), grid, dim3(WG_THREADS), lds, s, a);
    return hipGetLastError();
}

template <typename TO>
static hipError_t launch_compact_tile_t(int chain, int mode, const EvalArgs &a, dim3 grid, size_t lds, hipStream_t s) {
    switch (chain) {
        case CHAIN_TEMPLATE: return launch_compact_tile_c<CHAIN_TEMPLATE, TO>(mode, a, grid, lds, s);
        case CHAIN_SELF: return launch_compact_tile_c<CHAIN_SELF, TO>(mode, a, grid, lds, s);
        default: return launch_compact_tile_c<CHAIN_FREE, TO>(mode, a, grid, lds, s);
    }
}

template <int CHAIN>
static hipError_t launch_compact_c(int mode, const EvalArgs &a, dim3 grid, hipStream_t s) {
    if (mode == MODE_RESID) hipLaunchKernelGGL((ba_compact_kernel<CHAIN, MODE_RESID>), grid, dim3(WG_THREADS), 0, s, a);
    else if (mode == MODE_JAC) hipLaunchKernelGGL((ba_compact_kernel<CHAIN, MODE_JAC>), grid, dim3(WG_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ba_compact_kernel<CHAIN, MODE_RESID | MODE_JAC>), grid, dim3(WG_THREADS), 0, s, a);
    return hipGetLastError();
}

static hipError_t launch_compact_t(int chain, int mode, const EvalArgs &a, dim3 grid, hipStream_t s) {
    switch (chain) {
        case CHAIN_TEMPLATE: return launch_compact_c<CHAIN_TEMPLATE>(mode, a, grid, s);
        case CHAIN_SELF: return launch_compact_c<CHAIN_SELF>(mode, a, grid, s);
        default: return launch_compact_c<CHAIN_FREE>(mode, a, grid, s);
    }
}

static int launch_slab_prep(pcs_engine *h, const double *d_prm, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
    HIPCHK(order_after_done(h, s));   // the slabs are shared: an evaluation still reading them on another stream goes first
    const int has_pose = h->chain != PCS_CHAIN_FREE;
    const int copy_points = h->chain != PCS_CHAIN_TEMPLATE;
    int64_t threads = slab_prep_threads(h->n_cams, h->n_imgs, has_pose);   // one per slab element
    if (copy_points) threads = std::max<int64_t>(threads, std::min<int64_t>(3 * h->n_keys, 1 << 16));
    const dim3 grid((unsigned)((threads + 63) / 64));
    hipExtLaunchKernelGGL(slab_prep_kernel, grid, dim3(64), 0, s, start, stop, 0, d_prm, h->d_cam_slab.as<double>(),
                          h->d_pose_slab.as<double>(), h->d_points.as<double>(), (int)h->n_cams, (int)h->n_imgs, (int)h->n_keys,
                          h->extr_off, h->pose_off, h->point_off, has_pose, copy_points);
    HIPCHK(hipGetLastError());
    h->linearized = true;
    return PCS_OK;
}

template <int CHAIN, bool LDS_ACC>
static hipError_t launch_matfree_c(int op, const MatfreeArgs &a, dim3 grid, size_t lds, hipStream_t s) {
    if (lds > 48 * 1024) {  // opt in to more than the default dynamic-LDS cap
        const void *fns[] = {(const void *)ba_matfree_kernel<CHAIN, OP_JTU, LDS_ACC>, (const void *)ba_matfree_kernel<CHAIN, OP_JTJV, LDS_ACC>,
                             (const void *)ba_matfree_kernel<CHAIN, OP_DIAG, LDS_ACC>, (const void *)ba_matfree_kernel<CHAIN, OP_GRAD, LDS_ACC>};
        hipError_t e = hipFuncSetAttribute(fns[op - 1], hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    switch (op) {
        case OP_JV: hipLaunchKernelGGL((ba_matfree_kernel<CHAIN, OP_JV, false>), grid, dim3(256), 0, s, a); break;
        case OP_JTU: hipLaunchKernelGGL((ba_matfree_kernel<CHAIN, OP_JTU, LDS_ACC>), grid, dim3(256), lds, s, a); break;
        case OP_JTJV: hipLaunchKernelGGL((ba_matfree_kernel<CHAIN, OP_JTJV, LDS_ACC>), grid, dim3(256), lds, s, a); break;
        case OP_DIAG: hipLaunchKernelGGL((ba_matfree_kernel<CHAIN, OP_DIAG, LDS_ACC>), grid, dim3(256), lds, s, a); break;
        default: hipLaunchKernelGGL((ba_matfree_kernel<CHAIN, OP_GRAD, LDS_ACC>), grid, dim3(256), lds, s, a); break;
    }
    return hipGetLastError();
}

static hipError_t launch_matfree_t(int chain, int op, bool lds_acc, const MatfreeArgs &a, dim3 grid, size_t lds, hipStream_t s) {
    if (lds_acc) {
        switch (chain) {
            case CHAIN_TEMPLATE: return launch_matfree_c<CHAIN_TEMPLATE, true>(op, a, grid, lds, s);
            case CHAIN_SELF: return launch_matfree_c<CHAIN_SELF, true>(op, a, grid, lds, s);
            default: return launch_matfree_c<CHAIN_FREE, true>(op, a, grid, lds, s);
        }
    }
    switch (chain) {
        case CHAIN_TEMPLATE: return launch_matfree_c<CHAIN_TEMPLATE, false>(op, a, grid, 0, s);
        case CHAIN_SELF: return launch_matfree_c<CHAIN_SELF, false>(op, a, grid, 0, s);
        default: return launch_matfree_c<CHAIN_FREE, false>(op, a, grid, 0, s);
    }
}

// one pass of the normal-equations kernel (ba_normal.hpp); the workgroup is one wave
template <int CHAIN, int PASS>
static hipError_t launch_normal_p(int rows, const NormalArgs &a, dim3 grid, hipStream_t s) {
    if (rows == 32) hipLaunchKernelGGL((ba_normal_mfma_kernel<CHAIN, PASS, 32>), grid, dim3(64), normal_lds_bytes(CHAIN, PASS, 32), s, a);
    else hipLaunchKernelGGL((ba_normal_mfma_kernel<CHAIN, PASS, 64>), grid, dim3(64), normal_lds_bytes(CHAIN, PASS, 64), s, a);
    return hipGetLastError();
}

static hipError_t launch_normal(int chain, int pass, int rows, const NormalArgs &a, dim3 grid, hipStream_t s) {
    if (pass == PASS_SHARED) {
        switch (chain) {
            case CHAIN_TEMPLATE: return launch_normal_p<CHAIN_TEMPLATE, PASS_SHARED>(rows, a, grid, s);
            case CHAIN_SELF: return launch_normal_p<CHAIN_SELF, PASS_SHARED>(rows, a, grid, s);
            default: return launch_normal_p<CHAIN_FREE, PASS_SHARED>(rows, a, grid, s);
        }
    }
    if (pass == PASS_CAMKEY)
        return chain == CHAIN_SELF ? launch_normal_p<CHAIN_SELF, PASS_CAMKEY>(rows, a, grid, s) : launch_normal_p<CHAIN_FREE, PASS_CAMKEY>(rows, a, grid, s);
    return launch_normal_p<CHAIN_SELF, PASS_IMGKEY>(rows, a, grid, s);
}

// dst[i] = src[order[i]] (one-off, at the first normal-equations call)
template <typename E>
__global__ void gather_rows_kernel(const int32_t *__restrict__ order, const E *__restrict__ src, E *__restrict__ dst, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[order[i]];
}
template <typename E>
static hipError_t gather_rows(const int32_t *order, const void *src, void **dst, int64_t n, hipStream_t s) {
    hipError_t e = hipMalloc(dst, sizeof(E) * n);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gather_rows_kernel<E>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, order, static_cast<const E *>(src), static_cast<E *>(*dst), n);
    return hipGetLastError();
}

// (cam, key)- and (image, key)-sorted visiting orders for the point passes of the normal equations: built on the host
// at the first normal-equations call of a self / free engine (two stable sorts, ~0.1 s at 1e6 detections)
static int build_point_orders(pcs_engine *h) {
    const int64_t n = h->det.n;
    if (n <= 0) return PCS_OK;
    if (h->chain != PCS_CHAIN_TEMPLATE) {
        std::vector<int32_t> order(n);
        for (int pass = 0; pass < (h->chain == PCS_CHAIN_SELF ? 2 : 1); ++pass) {
            const std::vector<int32_t> &major = pass == 0 ? h->det.h.cam : h->det.h.img;
            for (int64_t i = 0; i < n; ++i) order[i] = (int32_t)i;
            std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
                return major[x] != major[y] ? major[x] < major[y] : h->det.h.key[x] < h->det.h.key[y];
            });
            DevBuf &dst = pass == 0 ? h->d_order_ck : h->d_order_ik;
            if (const int rc = dst.grow(n, sizeof(int32_t))) return rc;
            HIPCHK(hipMemcpy(dst.p, order.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice));
            if (pass == 0) h->h_order_ck = order;
        }
    }
    // the table in each visiting order: the shared pass of a scattered table, the (cam, key) pass, the (image, key) pass (which
    // reads no measurements)
    const int32_t *orders[3] = {h->d_order.as<int32_t>(), h->d_order_ck.as<int32_t>(), h->d_order_ik.as<int32_t>()};
    using u2 = __attribute__((ext_vector_type(2))) uint32_t;
    using u4 = __attribute__((ext_vector_type(4))) uint32_t;
    for (int pass = 0; pass < 3; ++pass) {
        if (!orders[pass]) continue;
        void **t = h->d_sorted[pass];
        if (h->det.packed.p) {
            HIPCHK(gather_rows<uint32_t>(orders[pass], h->det.packed.p, &t[0], n, h->stream));
        } else {
            HIPCHK(gather_rows<uint32_t>(orders[pass], h->det.cam.p, &t[1], n, h->stream));
            HIPCHK(gather_rows<uint32_t>(orders[pass], h->det.img.p, &t[2], n, h->stream));
            HIPCHK(gather_rows<uint32_t>(orders[pass], h->det.key.p, &t[3], n, h->stream));
        }
        if (pass != PASS_IMGKEY) HIPCHK(h->msize == 4 ? gather_rows<u2>(orders[pass], h->det.uv.p, &t[4], n, h->stream) : gather_rows<u4>(orders[pass], h->det.uv.p, &t[4], n, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return PCS_OK;
}

// all or nothing: a build that fails half-way (an allocation, a gather launch) leaves no sorted copy behind, so that the
// next call starts again instead of pairing sorted index words with unsorted measurements
static int ensure_point_orders(pcs_engine *h) {
    if (h->point_orders_tried) return PCS_OK;
    const int rc = build_point_orders(h);
    if (rc == PCS_OK) {
        h->point_orders_tried = true;
        return PCS_OK;
    }
    const std::string keep = g_err;
    (void)hipStreamSynchronize(h->stream);
    h->d_order_ck.release();
    h->d_order_ik.release();
    free_sorted_tables(h);
    g_err = keep;
    return rc;
}

// The (image, key) pass reads no measurements under the linear loss, so build_point_orders gathers none for it; a robust loss weighs
// the pass's rows by their residuals, and the first build with one gathers the measurements into that order as well (kept with the table).
// The gather is queued on the BUILD's stream `s`, in front of the pass that reads it; later work on any other stream is ordered behind
// the build's `done` event (enqueue_normal's mark_done, order_after_done of the next enqueue) like every other output of the build.
static int ensure_imgkey_uv(pcs_engine *h, hipStream_t s) {
    void **t = h->d_sorted[PASS_IMGKEY];
    if (t[4] || !h->d_order_ik.p || h->det.n <= 0) return PCS_OK;
    using u2 = __attribute__((ext_vector_type(2))) uint32_t;
    using u4 = __attribute__((ext_vector_type(4))) uint32_t;
    hipError_t e = h->msize == 4 ? gather_rows<u2>(h->d_order_ik.as<int32_t>(), h->det.uv.p, &t[4], h->det.n, s) : gather_rows<u4>(h->d_order_ik.as<int32_t>(), h->det.uv.p, &t[4], h->det.n, s);
    if (e != hipSuccess) {
        if (t[4]) (void)hipFree(t[4]);
        t[4] = nullptr;
        return fail(PCS_ERR_HIP, "robust loss: gathering the measurements of the (image, key) pass failed: %s", hipGetErrorString(e));
    }
    return PCS_OK;
}

// Noise weights (pcs_set_weights) in the visiting order of `pass`, beside the pass's sorted index words and measurements: gathered at the first
// weighted build after they were set, on the build's stream like ensure_imgkey_uv's measurements, and kept until the weights or the table change.
static int ensure_sorted_weights(pcs_engine *h, int pass, const int32_t *order, hipStream_t s) {
    void **t = h->d_sorted[pass];
    if (t[5] || !h->det.w.p || !order || h->det.n <= 0) return PCS_OK;
    const hipError_t e = gather_rows<uint64_t>(order, h->det.w.p, &t[5], h->det.n, s);
    if (e != hipSuccess) {
        if (t[5]) (void)hipFree(t[5]);
        t[5] = nullptr;
        return fail(PCS_ERR_HIP, "noise weights: gathering them into the visiting order of pass %d failed: %s", pass, hipGetErrorString(e));
    }
    return PCS_OK;
}

// ---- deterministic mode: the static tables of the ordered second pass (csrc/ba_reduce.hpp) ---------------------------------------------
// For MFMA pass `pass` (0 shared, 1 (cam, key)) walked with `tpw` tiles per wave: segments = maximal stretches of detections inside one
// run and one wave; logical runs = the segments of one key pair (one stretch in a sorted table; several when a pair re-appears);
// groups = up to RED_RUNS_PER_GROUP logical runs of one camera; per camera its groups, per entity (image / key) its runs in camera order.
static int ensure_det_tables(pcs_engine *h, int pass, int64_t tpw) {
    pcs_engine::DetPass &D = h->det_pass[pass];
    if (D.n == h->det.n && D.tpw == tpw && D.d_idx) return PCS_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(wait_done_host(h));
    if (D.d_idx) (void)hipFree(D.d_idx);
    if (D.d_work) (void)hipFree(D.d_work);
    D = pcs_engine::DetPass{};
    const int64_t n = h->det.n;
    const bool has_pose = h->chain != PCS_CHAIN_FREE;
    const std::vector<int32_t> *order = nullptr;
    if (pass == PASS_SHARED) { if (h->d_order.p) order = &h->h_order; }
    else order = &h->h_order_ck;
    if (order && (int64_t)order->size() != n) return fail(PCS_ERR_STATE, "deterministic mode: the host copy of a visiting order is missing");
    auto key_of = [&](int64_t d, int32_t &ka, int32_t &kb) {
        const int64_t i = order ? (*order)[d] : d;
        ka = h->det.h.cam[i];
        kb = pass == PASS_SHARED ? (has_pose ? h->det.h.img[i] : 0) : h->det.h.key[i];
    };
    const int64_t per_wave = tpw * TILE;
    const int64_t n_waves = (n + per_wave - 1) / per_wave;
    std::vector<int32_t> seg_base((size_t)n_waves), seg_ka, seg_kb;
    {
        int32_t pa = -1, pb = -1;
        for (int64_t d = 0; d < n; ++d) {
            int32_t ka, kb;
            key_of(d, ka, kb);
            const bool wave_start = d % per_wave == 0;
            if (wave_start) seg_base[(size_t)(d / per_wave)] = (int32_t)seg_ka.size();
            if (wave_start || ka != pa || kb != pb) {
                if (seg_ka.size() >= (size_t)INT32_MAX - 1) return fail(PCS_ERR_ARG, "deterministic mode: too many segments");
                seg_ka.push_back(ka);
                seg_kb.push_back(kb);
            }
            pa = ka;
            pb = kb;
        }
    }
    const int64_t n_seg = (int64_t)seg_ka.size();
    // logical runs: segments sorted by (ka, kb), table order inside one pair
    std::vector<int32_t> lr_segs((size_t)n_seg);
    for (int64_t i = 0; i < n_seg; ++i) lr_segs[(size_t)i] = (int32_t)i;
    std::stable_sort(lr_segs.begin(), lr_segs.end(), [&](int32_t x, int32_t y) {
        return seg_ka[x] != seg_ka[y] ? seg_ka[x] < seg_ka[y] : seg_kb[x] < seg_kb[y];
    });
    // the free chain's shared pass has one run per camera and owns camera-level entries only: a long run may be cut into pieces
    const bool may_split = pass == PASS_SHARED && !has_pose;
    std::vector<int32_t> lr_ptr, lr_ka, lr_kb;
    for (int64_t i = 0; i < n_seg; ++i) {
        const int32_t sgm = lr_segs[(size_t)i];
        const bool fresh = i == 0 || seg_ka[sgm] != lr_ka.back() || seg_kb[sgm] != lr_kb.back() ||
                           (may_split && i - lr_ptr.back() >= RED_SPLIT_SEGS);
        if (fresh) {
            lr_ptr.push_back((int32_t)i);
            lr_ka.push_back(seg_ka[sgm]);
            lr_kb.push_back(seg_kb[sgm]);
        }
    }
    const int64_t n_lr = (int64_t)lr_ka.size();
    lr_ptr.push_back((int32_t)n_seg);
    std::vector<int32_t> grp_ptr, cam_ptr((size_t)h->n_cams + 1, 0);
    for (int64_t r = 0; r < n_lr; ++r) {
        const bool fresh = r == 0 || lr_ka[(size_t)r] != lr_ka[(size_t)r - 1] || r - grp_ptr.back() >= RED_RUNS_PER_GROUP;
        if (fresh) {
            grp_ptr.push_back((int32_t)r);
            ++cam_ptr[(size_t)lr_ka[(size_t)r] + 1];
        }
    }
    const int64_t n_grp = (int64_t)grp_ptr.size();
    grp_ptr.push_back((int32_t)n_lr);
    for (int64_t c = 0; c < h->n_cams; ++c) cam_ptr[(size_t)c + 1] += cam_ptr[(size_t)c];
    const bool has_ent = pass == PASS_CAMKEY || has_pose;
    const int64_t n_ent = !has_ent ? 0 : pass == PASS_SHARED ? h->n_imgs : h->n_keys;
    std::vector<int32_t> ent_ptr((size_t)n_ent + 1, 0), ent_runs(has_ent ? (size_t)n_lr : 0);
    if (has_ent) {
        for (int64_t r = 0; r < n_lr; ++r) ++ent_ptr[(size_t)lr_kb[(size_t)r] + 1];
        for (int64_t e = 0; e < n_ent; ++e) ent_ptr[(size_t)e + 1] += ent_ptr[(size_t)e];
        std::vector<int32_t> fill(ent_ptr.begin(), ent_ptr.end() - 1);
        for (int64_t r = 0; r < n_lr; ++r) ent_runs[(size_t)fill[(size_t)lr_kb[(size_t)r]]++] = (int32_t)r;   // runs are sorted by camera: camera order per entity
    }
    const std::vector<int32_t> *parts[9] = {&seg_base, &lr_ptr, &lr_segs, &lr_ka, &lr_kb, &grp_ptr, &cam_ptr, &ent_ptr, &ent_runs};
    int64_t total = 0;
    for (int i = 0; i < 9; ++i) {
        D.off[i] = total;
        total += ((int64_t)parts[i]->size() + 3) & ~(int64_t)3;
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMalloc(&D.d_idx, sizeof(int32_t) * std::max<int64_t>(total, 4)));
    for (int i = 0; i < 9; ++i)
        if (!parts[i]->empty()) HIPCHK(hipMemcpy(D.d_idx + D.off[i], parts[i]->data(), sizeof(int32_t) * parts[i]->size(), hipMemcpyHostToDevice));
    const int nm = (pass == PASS_SHARED && has_pose) ? 2 : 1;
    D.work_off[0] = 0;
    D.work_off[1] = n_seg * nm * 256;
    D.work_off[2] = D.work_off[1] + n_lr * RED_Q;
    D.work_off[3] = D.work_off[2] + n_grp * RED_G + 2;
    HIPCHK(hipMalloc(&D.d_work, sizeof(double) * (size_t)(D.work_off[3] + n_waves)));
    D.n = n; D.tpw = tpw;
    D.n_seg = (int32_t)n_seg; D.n_lr = (int32_t)n_lr; D.n_grp = (int32_t)n_grp; D.n_ent = (int32_t)n_ent; D.n_waves = (int32_t)n_waves;
    return PCS_OK;
}

template <int CHAIN, int PASS>
static hipError_t launch_reduce_p(const NormalArgs &a, const ReduceArgs &ra, hipStream_t s) {
    static_assert(RED_RUNS_PER_GROUP == 4, "one wave per run, four waves per workgroup");
    if (ra.n_grp > 0) hipLaunchKernelGGL((normal_reduce_runs_kernel<CHAIN, PASS>), dim3((unsigned)ra.n_grp), dim3(256), 0, s, a, ra);
    const int blocks = (PASS == PASS_SHARED ? ra.n_cams + 1 : 0) + (ra.n_ent + 2) / 3;
    if (blocks > 0) hipLaunchKernelGGL((normal_reduce_final_kernel<CHAIN, PASS>), dim3((unsigned)blocks), dim3(256), 0, s, a, ra);
    return hipGetLastError();
}
static hipError_t launch_reduce(int chain, int pass, const NormalArgs &a, const ReduceArgs &ra, hipStream_t s) {
    if (pass == PASS_SHARED) {
        switch (chain) {
            case CHAIN_TEMPLATE: return launch_reduce_p<CHAIN_TEMPLATE, PASS_SHARED>(a, ra, s);
            case CHAIN_SELF: return launch_reduce_p<CHAIN_SELF, PASS_SHARED>(a, ra, s);
            default: return launch_reduce_p<CHAIN_FREE, PASS_SHARED>(a, ra, s);
        }
    }
    return chain == CHAIN_SELF ? launch_reduce_p<CHAIN_SELF, PASS_CAMKEY>(a, ra, s) : launch_reduce_p<CHAIN_FREE, PASS_CAMKEY>(a, ra, s);
}

static BlockLayout block_layout(const pcs_engine *h) {
    BlockLayout L{};
    if (h->chain == PCS_CHAIN_TEMPLATE) { L.tg = 2; L.tb = 6; L.trail_off = h->pose_off; L.n_ent = h->n_imgs; }
    else { L.tg = 3; L.tb = 3; L.trail_off = h->point_off; L.n_ent = h->n_keys; }
    L.n_lead = L.trail_off;
    L.n_trail = L.n_ent * L.tb;
    return L;
}

// slab_prep + the normal-equations passes on `s`; d_prm holds the parameter string; outputs are zeroed here.
// blocked: d_H points at the packed [A | B | C] (contiguous), see pcs_normal_blocks_device.
// What a build inside an LM trial adds: the stop flag; sel (LM loop with two states, ba_schur.hpp SchurArgs::sel): when *sel != 0 the string is read
// alt_prm doubles and the outputs are written alt_out doubles further on; skip_prologue: the launch in front has prepared the slabs and zeroed the outputs.
struct NormalTrial { const int32_t *stop = nullptr, *sel = nullptr; int64_t alt_prm = 0, alt_out = 0; bool skip_prologue = false; };
static int enqueue_normal(pcs_engine *h, const double *d_prm, double *d_H, double *d_g, double *d_cost, hipStream_t s, bool blocked = false, const NormalTrial &t = {}) {
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    if (h->det.n > INT32_MAX) return fail(PCS_ERR_ARG, "normal equations: tables beyond 2^31 rows are not supported (visiting orders are int32)");
    if (h->chain == PCS_CHAIN_TEMPLATE && !h->have_template) return fail(PCS_ERR_STATE, "template points not set");
    const BlockLayout L = block_layout(h);
    if (!blocked) {
        // the flush addresses H with 32-bit offsets in doubles: n^2 < 2^32 (a 34 GB matrix)
        if (h->n_params > PCS_NORMAL_MAX_PARAMS) return fail(PCS_ERR_ARG, "normal equations: more than %d parameters (dense H beyond 32 GiB) is not supported", PCS_NORMAL_MAX_PARAMS);
    } else {
        const int64_t lim = (int64_t)1 << 32;   // doubles per region: 32-bit offsets in doubles (32 GiB; rounds 3-4: byte offsets, 4 GiB)
        if (L.a_len() >= lim || L.b_len() >= lim || L.c_len() >= lim)
            return fail(PCS_ERR_ARG, "blocked normal equations: a region beyond 32 GiB (leading %lld, trailing %lld columns) is not supported; use pcs_matfree",
                        (long long)L.n_lead, (long long)L.n_trail);
    }
    HIPCHK(hipSetDevice(h->device));
    int rc0 = ensure_point_orders(h);
    if (rc0) return rc0;
    if ((t.stop || t.sel) && (reinterpret_cast<uintptr_t>(d_H) % 16 || t.alt_out % 2)) return fail(PCS_ERR_ARG, "normal equations behind a stop flag / state selector need 16-byte aligned buffers");
    if (t.skip_prologue) {   // the caller's previous kernel has prepared the slabs and zeroed the outputs (schur_finish_kernel, csrc/ba_lm_fused.hpp)
        HIPCHK(order_after_done(h, s));
        h->linearized = true;
    } else if (reinterpret_cast<uintptr_t>(d_H) % 16 == 0) {   // slab_prep and the zeroing of the outputs in one launch
        HIPCHK(order_after_done(h, s));
        const int has_pose = h->chain != PCS_CHAIN_FREE, copy_points = h->chain != PCS_CHAIN_TEMPLATE;
        int64_t threads = slab_prep_threads(h->n_cams, h->n_imgs, has_pose);
        if (copy_points) threads = std::max<int64_t>(threads, std::min<int64_t>(3 * h->n_keys, 1 << 16));
        const int prep_blocks = (int)((threads + 63) / 64);
        const int64_t n_h = blocked ? L.h_len() : h->n_params * h->n_params;
        const int zero_blocks = (int)std::min<int64_t>((n_h / 2 + 63) / 64 + 1, (int64_t)h->n_cu * 32);
        hipLaunchKernelGGL(normal_prologue_kernel, dim3((unsigned)(prep_blocks + zero_blocks)), dim3(64), 0, s, d_prm, h->d_cam_slab.as<double>(),
                           h->d_pose_slab.as<double>(), h->d_points.as<double>(), (int)h->n_cams, (int)h->n_imgs, (int)h->n_keys, h->extr_off,
                           h->pose_off, h->point_off, has_pose, copy_points, prep_blocks, d_H, n_h, d_g, h->n_params, d_cost, t.stop, t.sel, t.alt_prm, t.alt_out);
        HIPCHK(hipGetLastError());
        h->linearized = true;
    } else {
        HIPCHK(hipMemsetAsync(d_H, 0, sizeof(double) * (blocked ? L.h_len() : h->n_params * h->n_params), s));
        HIPCHK(hipMemsetAsync(d_g, 0, sizeof(double) * h->n_params, s));
        HIPCHK(hipMemsetAsync(d_cost, 0, sizeof(double), s));
        int rc = launch_slab_prep(h, d_prm, s);
        if (rc) return rc;
    }
    NormalArgs a{};
    a.tab = h->det.table();
    a.cam_slab = h->d_cam_slab.p; a.pose_slab = h->d_pose_slab.p; a.points = h->d_points.p;
    a.H = d_H; a.g = d_g; a.cost = d_cost;
    if (blocked) {
        a.HB = d_H + L.a_len(); a.HC = a.HB + L.b_len();
        a.ldA = (int32_t)L.n_lead; a.ldB = (int32_t)L.n_trail; a.tb = L.tb; a.trail_group = L.tg; a.trail_off = L.trail_off;
    } else {
        a.HB = a.HC = d_H;
        a.ldA = (int32_t)h->n_params; a.ldB = 0; a.tb = 0; a.trail_group = -1; a.trail_off = 0;
    }
    a.n = h->det.n; a.n_tiles = (h->det.n + TILE - 1) / TILE;
    a.extr_off = h->extr_off; a.pose_off = h->pose_off; a.point_off = h->point_off;
    a.n_params = h->n_params;
    a.debug = h->normal_debug;
    a.loss = h->loss; a.inv_f_scale = 1.0 / h->f_scale; a.f_scale_sq = h->f_scale * h->f_scale;
    const bool weighted = h->det.w.p != nullptr;   // noise weights: the robust path, with the linear kind when no loss is set (f_scale plays no part)
    if (weighted && h->loss == LOSS_LINEAR) a.loss = LOSS_LINEAR_WHITENED, a.inv_f_scale = a.f_scale_sq = 1.0;
    a.stop = t.stop;
    a.sel = t.sel; a.alt = t.alt_out;
    // every wave walks a contiguous range of tiles, so its register accumulators survive across tiles.  One-wave
    // workgroups; the LDS image (22.9 KB for 22 columns x 64 rows) allows 7 per CU, and exactly one resident round of
    // waves is fastest (92 us against 105 us with two rounds on rig-32, profiles/r02/sweeps.md).
    // Tables of 1 024 - 1 792 tiles: two tiles per wave instead of one.  A wave flushes everything it holds when it ends, and with
    // one tile per wave every tile pays the camera-level flush into addresses that hundreds of waves share (ring-8, 1 600 tiles,
    // 8 cameras: 35.0 us at one tile per wave, 27.7 at two, 28.4 at three).  Smaller tables keep one tile per wave: there the
    // second tile's latency costs more than the flushes (110 tiles: 14.4 against 20.4 us).
    auto geometry = [&](const int64_t wpc, const int64_t min_tiles = 1) {
        const int64_t target_waves = (int64_t)h->n_cu * wpc;
        const int64_t tpw = std::max<int64_t>(std::min<int64_t>(min_tiles, a.n_tiles), (a.n_tiles + target_waves - 1) / target_waves);
        a.tiles_per_wave = (int32_t)tpw;
        return dim3((unsigned)((a.n_tiles + tpw - 1) / tpw));
    };
    // start / stop events of the passes (pcs_last_kernel_ms) unless timing is switched off: an event record is a packet of its own
    // between two launches, ~5 us each on the stream (the device LM loop builds once per trial and switches them off)
    const bool timed = h->timing_every > 0;
    hipEvent_t *ev = timed ? ring_slot(h, false) : nullptr;
    if (timed) HIPCHK(hipEventRecord(ev[2], s));
    const int n_pass = h->chain == PCS_CHAIN_TEMPLATE ? 1 : h->chain == PCS_CHAIN_SELF ? 3 : 2;
    for (int pass = 0; pass < n_pass; ++pass) {
        if (h->normal_debug & (256 << pass)) continue;   // profiling: time the passes one by one
        a.order = pass == PASS_SHARED ? h->d_order.as<int32_t>() : pass == PASS_CAMKEY ? h->d_order_ck.as<int32_t>() : h->d_order_ik.as<int32_t>();
        if (pass != PASS_SHARED && !a.order) return fail(PCS_ERR_STATE, "normal equations: key-sorted visiting order missing");
        a.tab = h->det.table();
        a.inv_sigma = h->det.w.as<const double>();   // table order, read through a.order like the table itself
        if (a.order && h->sort_tables) {   // the pass's own copy of the table, already in visiting order
            if (pass == PASS_IMGKEY && (h->loss || weighted)) {   // a robust loss (noise weights) weighs the (image, key) pass's rows by their residuals: it needs the measurements too
                const int rc = ensure_imgkey_uv(h, s);
                if (rc) return rc;
            }
            void *const *t = h->d_sorted[pass];
            const bool have_table = (t[0] || t[1]) && (t[4] || pass == PASS_IMGKEY);   // index words AND measurements, or neither
            if (have_table && weighted) {
                const int rc = ensure_sorted_weights(h, pass, a.order, s);
                if (rc) return rc;
            }
            if (have_table) {
                a.tab.packed = static_cast<const uint32_t *>(t[0]);
                a.tab.cam = static_cast<const int32_t *>(t[1]); a.tab.img = static_cast<const int32_t *>(t[2]); a.tab.key = static_cast<const int32_t *>(t[3]);
                if (t[4]) a.tab.uv = t[4];
                if (weighted) a.inv_sigma = static_cast<const double *>(t[5]);   // ... and the weights in the same order
                a.order = nullptr;
            }
        }
        hipError_t e;
        a.part = nullptr; a.seg_base = nullptr; a.wave_cost = nullptr;
        if (pass == PASS_IMGKEY && h->deterministic) {
            // this pass keeps its atomics: a run is at most n_cams long, so with n_cams <= 64 no address gets more than two contributions
            // (csrc/ba_reduce.hpp) — beyond that the order of three could show in the last bit
            if (h->n_cams > 64) return fail(PCS_ERR_ARG, "deterministic mode: the (image, key) pass of the self chain supports at most 64 cameras (%lld)", (long long)h->n_cams);
        }
        if (pass == PASS_IMGKEY && (h->normal_imgkey_product || h->deterministic)) {
            // 7 KB of LDS and 167 VGPRs per wave: 12 resident per CU.  The kernel waits on dependent loads and on its
            // atomics, so short waves (one or two tiles each, 48 per CU) that keep every slot refilled are fastest
            // (59 / 56 / 55 / 59 us for 12 / 24 / 48 / 96 per CU at N = 1e6, profiles/r02/sweeps.md)
            const dim3 grid = geometry(h->normal_imgkey_wgs_per_cu > 0 ? h->normal_imgkey_wgs_per_cu : 48);
            hipLaunchKernelGGL(ba_normal_imgkey_kernel, grid, dim3(64), normal_imgkey_lds_bytes(), s, a);
            e = hipGetLastError();
        } else {
            // the shared pass's image (22.9 KB) allows 7 waves per CU; the (cam, key) pass's (19.8 KB) allows 8 = two per SIMD,
            // 65.5 against 70.0 us on rig-32-self (profiles/r02/sweeps.md)
            const dim3 grid = geometry(h->wgs_per_cu > 0 ? h->wgs_per_cu : pass == PASS_CAMKEY ? 8 : 7, (h->wgs_per_cu > 0 || a.n_tiles < 1024) ? 1 : 2);
            if (h->deterministic) {   // the kernel stores its finished accumulators per segment, an ordered second pass sums them (csrc/ba_reduce.hpp)
                const int rc = ensure_det_tables(h, pass, a.tiles_per_wave);
                if (rc) return rc;
                const pcs_engine::DetPass &D = h->det_pass[pass];
                if ((int64_t)grid.x != D.n_waves) return fail(PCS_ERR_STATE, "deterministic mode: launch geometry and segment table disagree");
                a.part = D.d_work + D.work_off[0];
                a.seg_base = D.d_idx + D.off[0];
                a.wave_cost = D.d_work + D.work_off[3];
                e = launch_normal(h->chain, pass, h->normal_rows, a, grid, s);
                if (e == hipSuccess) {
                    ReduceArgs ra{};
                    ra.part = a.part; ra.Q = D.d_work + D.work_off[1]; ra.G = D.d_work + D.work_off[2];
                    ra.lr_ptr = D.d_idx + D.off[1]; ra.lr_segs = D.d_idx + D.off[2]; ra.lr_ka = D.d_idx + D.off[3]; ra.lr_kb = D.d_idx + D.off[4];
                    ra.grp_ptr = D.d_idx + D.off[5]; ra.cam_ptr = D.d_idx + D.off[6]; ra.ent_ptr = D.d_idx + D.off[7]; ra.ent_runs = D.d_idx + D.off[8];
                    ra.n_lr = D.n_lr; ra.n_grp = D.n_grp; ra.n_cams = (int32_t)h->n_cams; ra.n_ent = D.n_ent; ra.n_waves = D.n_waves;
                    e = launch_reduce(h->chain, pass, a, ra, s);
                }
            } else {
                e = launch_normal(h->chain, pass, h->normal_rows, a, grid, s);
            }
        }
        if (e != hipSuccess) return fail(PCS_ERR_HIP, "normal-equations kernel launch failed: %s", hipGetErrorString(e));
    }
    if (timed) {
        HIPCHK(hipEventRecord(ev[3], s));
        ++h->ev_count;
        h->events_valid = true;
    }
    HIPCHK(mark_done(h, s));
    return PCS_OK;
}

// Queue slab_prep + the evaluation kernel on `s`.  d_prm must already hold the parameter string.
static int enqueue_eval(pcs_engine *h, const double *d_prm, void *d_resid, void *d_out, bool compact, hipStream_t s) {
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    if (h->chain == PCS_CHAIN_TEMPLATE && !h->have_template) return fail(PCS_ERR_STATE, "template points not set");
    const int mode = (d_resid ? MODE_RESID : 0) | (d_out ? MODE_JAC : 0);
    if (!mode) return PCS_OK;
    HIPCHK(hipSetDevice(h->device));
    // One launch per step for small, run-ordered tables (see pcs_engine::fuse_prep): the waves prepare their own slabs.
    const bool slab_lds_forced = h->variant >= 0 && (h->variant & VAR_SLAB_LDS);
    const bool prep = !compact && !slab_lds_forced && !(h->variant >= 0 && (mode & MODE_JAC) && !(h->variant & VAR_TRANSPOSE)) &&
                      (h->fuse_prep > 0 || (h->fuse_prep < 0 && h->tile_locality >= 0.5 && h->tile_segments <= 2.5 &&
                                            ((h->osize == 8 && (mode & MODE_JAC)) || h->det.n <= h->fuse_prep_max_n)));
    hipEvent_t no_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    const bool timed = h->timing_every > 0 && (h->eval_count++ % h->timing_every) == 0;
    hipEvent_t *ev = timed ? ring_slot(h, !prep) : no_ev;
    if (!prep) {
        int rc0 = launch_slab_prep(h, d_prm, s, ev[0], ev[1]);
        if (rc0) return rc0;
    } else {
        HIPCHK(order_after_done(h, s));   // keeps `done` meaning "everything queued so far", whatever stream it was on
        h->linearized = false;   // the global slabs are not refreshed: the matrix-free operators need pcs_linearize
    }
    EvalArgs a{};
    a.prm = d_prm; a.extr_off = h->extr_off; a.pose_off = h->pose_off; a.point_off = h->point_off;
    a.tab = h->det.table();
    a.cam_slab = h->d_cam_slab.p; a.pose_slab = h->d_pose_slab.p; a.points = h->d_points.p;
    a.resid = d_resid; a.jac = d_out; a.sink = h->d_sink.p;
    a.xcd_remap = h->xcd_remap ? 1 : 0;
    a.n = h->det.n; a.n_cams = (int32_t)h->n_cams; a.n_imgs = (int32_t)h->n_imgs; a.n_keys = (int32_t)h->n_keys;
    a.n_tiles = (h->det.n + TILE - 1) / TILE;
    if (compact) {
        a.keep = h->d_keep.as<uint32_t>(); a.row_off = h->d_row_off.as<int64_t>();
        if (timed) HIPCHK(hipEventRecord(ev[2], s));
        hipError_t e;
        if (h->compact_variant == 0 && h->dtype == PCS_F64) {  // per-lane stores (first version, kept for A/B)
            const int64_t blocks = std::min<int64_t>((h->det.n + WG_THREADS - 1) / WG_THREADS, (int64_t)h->n_cu * 8);
            e = launch_compact_t(h->chain, mode, a, dim3((unsigned)blocks), s);
        } else {
            const int64_t wpc = h->wgs_per_cu > 0 ? h->wgs_per_cu : 16;
            const int64_t target_wgs = (int64_t)h->n_cu * wpc;
            int64_t tpw = (a.n_tiles + target_wgs - 1) / target_wgs;
            tpw = std::max<int64_t>(WAVES_PER_WG, (tpw + WAVES_PER_WG - 1) / WAVES_PER_WG * WAVES_PER_WG);
            a.tiles_per_wg = (int32_t)tpw;
            const int64_t grid = (a.n_tiles + tpw - 1) / tpw;
            const size_t vs = 16 / h->osize;
            const size_t wave_lds = ((size_t)HALF * 2 * h->P + 128 / h->osize + 64 + vs - 1) / vs * vs;  // scalars, as in the kernel
            const size_t lds = (mode & MODE_JAC) ? h->osize * (size_t)WAVES_PER_WG * wave_lds : 0;
            e = h->osize == 8 ? launch_compact_tile_t<double>(h->chain, mode, a, dim3((unsigned)grid), lds, s)
                              : launch_compact_tile_t<float>(h->chain, mode, a, dim3((unsigned)grid), lds, s);
        }
        if (e != hipSuccess) return fail(PCS_ERR_HIP, "compact kernel launch failed: %s", hipGetErrorString(e));
        if (timed) HIPCHK(hipEventRecord(ev[3], s));
    } else {
        const bool local = h->tile_locality >= 0.5;
        int variant = h->variant >= 0 ? h->variant : (VAR_TRANSPOSE | VAR_NT | (local || prep ? 0 : VAR_SLAB_LDS));
        if (!(mode & MODE_JAC)) variant &= ~VAR_TRANSPOSE;
        // waves per workgroup: 4 for large tables; a small table (config 2: 1 600 tiles on 256 CUs) is cut into
        // one-wave workgroups so that every CU gets several and the tail of the grid stays short
        int waves = h->waves_per_wg;
        if (waves <= 0) waves = (variant & VAR_SLAB_LDS) ? WAVES_PER_WG : a.n_tiles >= (int64_t)h->n_cu * 32 ? WAVES_PER_WG : a.n_tiles >= (int64_t)h->n_cu * 16 ? 2 : 1;
        // LDS budget: slabs + points (+ one wave-private transpose region per wave)
        const size_t slab_bytes = sizeof(double) * (size_t)(h->n_cams * CAM_STRIDE + h->n_imgs * POSE_STRIDE + padded_points(h->n_keys));
        const size_t tr_bytes = (variant & VAR_TRANSPOSE) ? h->osize * (size_t)waves * HALF * lds_row_stride(2 * h->P, (int)h->osize) : 0;
        if ((variant & VAR_SLAB_LDS) && slab_bytes + tr_bytes > h->lds_limit) variant &= ~VAR_SLAB_LDS;  // read slabs through L1/L2
        const size_t lds = ((variant & VAR_SLAB_LDS) ? slab_bytes : 0) + (prep ? sizeof(double) * (size_t)waves * PAIR_SLAB : 0) + tr_bytes;
        int64_t tpw = h->tiles_per_wg;
        if (tpw <= 0 && h->wgs_per_cu <= 0 && !(variant & VAR_SLAB_LDS)) {
            // slabs through L1/L2: one tile per wave, as many workgroups as that takes.  Up to 1e6 detections this
            // is what 16 workgroups per CU give anyway; at 1e7 it beats 10 tiles per wave by 17 % (profiles/r01/sweeps.md)
            tpw = waves;
        } else if (tpw <= 0) {
            const int64_t wpc = h->wgs_per_cu > 0 ? h->wgs_per_cu : 2;  // LDS-staged slabs: few long-lived workgroups
            const int64_t target_wgs = (int64_t)h->n_cu * wpc;
            tpw = (a.n_tiles + target_wgs - 1) / target_wgs;
            tpw = std::max<int64_t>(waves, (tpw + waves - 1) / waves * waves);
        }
        a.tiles_per_wg = (int32_t)tpw;
        const int64_t grid = (a.n_tiles + tpw - 1) / tpw;
        const EvPair evp{ev[2], ev[3]};  // start / stop of the evaluation kernel itself
        hipError_t e = h->osize == 8 ? launch_eval_t<double>(h->chain, mode, variant, prep, a, dim3((unsigned)grid), 64 * waves, lds, s, evp)
                                     : launch_eval_t<float>(h->chain, mode, variant, prep, a, dim3((unsigned)grid), 64 * waves, lds, s, evp);
        if (e != hipSuccess) return fail(PCS_ERR_HIP, "eval kernel launch failed: %s", hipGetErrorString(e));
    }
    if (timed) {
        ++h->ev_count;
        h->events_valid = true;
    }
    HIPCHK(mark_done(h, s));
    return PCS_OK;
}

template <int CHAIN, int PASS>
static void fill_descriptors(int tg, int32_t *out) {
    for (int m = 0; m < 2; ++m)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) out[(m * 64 + lane) * 4 + r] = m < normal_mfmas(CHAIN, PASS) ? entry_descriptor<CHAIN, PASS>(m, lane, r, tg) : 0;
}

template <int CHAIN, int PASS>
static void fill_entry_map(int32_t *out) {
    for (int m = 0; m < 2; ++m)
        for (int lane = 0; lane < 64; ++lane)
            for (int r = 0; r < 4; ++r) {
                int sa = -1, sb = -1;
                const bool keep = m < normal_mfmas(CHAIN, PASS) && entry_kept<CHAIN, PASS>(m, (lane >> 4) + 4 * r, lane & 15, sa, sb);
                int32_t *o = out + ((m * 64 + lane) * 4 + r) * 2;
                o[0] = keep ? slot_col<CHAIN, PASS>(sa) : -1;
                o[1] = keep ? slot_col<CHAIN, PASS>(sb) : -1;
            }
}

static int stage_params(pcs_engine *h, const double *param_str, hipStream_t s) {
    // the pinned staging buffer is reused: wait until the previous copy out of it has been consumed
    HIPCHK(wait_done_host(h));
    memcpy(h->h_param, param_str, sizeof(double) * h->n_params);
    HIPCHK(hipMemcpyAsync(h->d_param.as<double>(), h->h_param, sizeof(double) * h->n_params, hipMemcpyHostToDevice, s));
    HIPCHK(mark_done(h, s));
    return PCS_OK;
}

static int ensure_scratch(pcs_engine *h, bool want_resid, bool want_jac, bool want_data) {
    HIPCHK(hipSetDevice(h->device));
    if (want_resid)   // doubles: the legacy cost of a mixed engine writes f64
        if (const int rc = h->d_resid.grow(2 * h->det.n, sizeof(double))) return rc;
    if (want_jac)
        if (const int rc = h->d_jac.grow(2 * h->det.n * h->P, h->osize)) return rc;
    if (want_data)
        if (const int rc = h->d_data.grow(std::max<int64_t>(1, h->nnz), h->osize)) return rc;
    return PCS_OK;
}

// device -> host as float64; `elem` = element size on the device (default: the engine's output type)
static int download(pcs_engine *h, double *dst, const void *d_src, int64_t count, hipStream_t s, size_t elem = 0) {
    if ((elem ? elem : h->osize) == 8) {
        HIPCHK(hipMemcpyAsync(dst, d_src, sizeof(double) * count, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    } else {
        std::vector<float> f(count);
        HIPCHK(hipMemcpyAsync(f.data(), d_src, sizeof(float) * count, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int64_t i = 0; i < count; ++i) dst[i] = (double)f[i];
    }
    return PCS_OK;
}

extern "C" {

int pcs_eval_device_resident(pcs_engine *h, const double *d_param_str, void *d_resid, void *d_jac, void *stream) {
    if (!h || !d_param_str) return fail(PCS_ERR_ARG, "pcs_eval_device_resident: bad arguments");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    return enqueue_eval(h, d_param_str, d_resid, d_jac, false, s);
}

int pcs_eval_device(pcs_engine *h, const double *param_str, void *d_resid, void *d_jac, void *stream) {
    if (!h || !param_str) return fail(PCS_ERR_ARG, "pcs_eval_device: bad arguments");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    HIPCHK(hipSetDevice(h->device));
    int rc = stage_params(h, param_str, s);
    if (rc) return rc;
    return enqueue_eval(h, h->d_param.as<double>(), d_resid, d_jac, false, s);
}

int pcs_eval(pcs_engine *h, const double *param_str, double *resid, double *jac) {
    if (!h || !param_str) return fail(PCS_ERR_ARG, "pcs_eval: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    int rc = ensure_scratch(h, resid != nullptr, jac != nullptr, false);
    if (rc) return rc;
    rc = pcs_eval_device(h, param_str, resid ? h->d_resid.p : nullptr, jac ? h->d_jac.p : nullptr, nullptr);
    if (rc) return rc;
    if (resid && (rc = download(h, resid, h->d_resid.p, 2 * h->det.n, h->stream))) return rc;
    if (jac && (rc = download(h, jac, h->d_jac.p, 2 * h->det.n * h->P, h->stream))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return PCS_OK;
}

int pcs_device_buffers(pcs_engine *h, void **d_resid, void **d_jac) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_device_buffers: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    int rc = ensure_scratch(h, d_resid != nullptr, d_jac != nullptr, false);
    if (rc) return rc;
    if (d_resid) *d_resid = h->d_resid.p;
    if (d_jac) *d_jac = h->d_jac.p;
    return PCS_OK;
}

int pcs_block_param_inds(pcs_engine *h, int64_t *out) {
    if (!h || !out) return fail(PCS_ERR_ARG, "pcs_block_param_inds: bad arguments");
    const int P = h->P;
    for (int64_t i = 0; i < h->det.n; ++i) {
        int64_t *o = out + i * P;
        const int64_t c = h->det.h.cam[i], im = h->det.h.img[i], k = h->det.h.key[i];
        int j = 0;
        for (int q = 0; q < 9; ++q) o[j++] = 9 * c + q;
        for (int q = 0; q < 6; ++q) o[j++] = h->extr_off + 6 * c + q;
        if (h->chain != PCS_CHAIN_FREE)
            for (int q = 0; q < 6; ++q) o[j++] = h->pose_off + 6 * im + q;
        if (h->chain != PCS_CHAIN_TEMPLATE)
            for (int q = 0; q < 3; ++q) o[j++] = h->point_off + 3 * k + q;
    }
    return PCS_OK;
}

// keep-mask of one detection's local columns under `unfixed`
static inline uint32_t keep_mask(const pcs_engine *h, const uint8_t *unfixed, int64_t i) {
    if (!unfixed) return (1u << h->P) - 1u;
    const int64_t c = h->det.h.cam[i], im = h->det.h.img[i], k = h->det.h.key[i];
    uint32_t m = 0;
    int j = 0;
    for (int q = 0; q < 9; ++q, ++j) m |= (uint32_t)(unfixed[9 * c + q] != 0) << j;
    for (int q = 0; q < 6; ++q, ++j) m |= (uint32_t)(unfixed[h->extr_off + 6 * c + q] != 0) << j;
    if (h->chain != PCS_CHAIN_FREE)
        for (int q = 0; q < 6; ++q, ++j) m |= (uint32_t)(unfixed[h->pose_off + 6 * im + q] != 0) << j;
    if (h->chain != PCS_CHAIN_TEMPLATE)
        for (int q = 0; q < 3; ++q, ++j) m |= (uint32_t)(unfixed[h->point_off + 3 * k + q] != 0) << j;
    return m;
}

int pcs_csr_structure(pcs_engine *h, const uint8_t *unfixed, int64_t *indices, int64_t *indptr, int64_t *nnz_out) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_csr_structure: bad arguments");
    // conversion = [0, cumsum(unfixed)]: full column -> free column (afb:482)
    std::vector<int64_t> conv(h->n_params + 1, 0);
    for (int64_t p = 0; p < h->n_params; ++p) conv[p + 1] = conv[p] + ((!unfixed || unfixed[p]) ? 1 : 0);
    std::vector<int64_t> cols(h->P);
    int64_t pos = 0;
    if (indptr) indptr[0] = 0;
    for (int64_t i = 0; i < h->det.n; ++i) {
        const int64_t c = h->det.h.cam[i], im = h->det.h.img[i], k = h->det.h.key[i];
        int j = 0;
        for (int q = 0; q < 9; ++q) cols[j++] = 9 * c + q;
        for (int q = 0; q < 6; ++q) cols[j++] = h->extr_off + 6 * c + q;
        if (h->chain != PCS_CHAIN_FREE)
            for (int q = 0; q < 6; ++q) cols[j++] = h->pose_off + 6 * im + q;
        if (h->chain != PCS_CHAIN_TEMPLATE)
            for (int q = 0; q < 3; ++q) cols[j++] = h->point_off + 3 * k + q;
        for (int row = 0; row < 2; ++row) {  // each detection's index row is used for u and for v (afb:475-479)
            for (int q = 0; q < h->P; ++q) {
                if (!unfixed || unfixed[cols[q]]) {
                    if (indices) indices[pos] = conv[cols[q]];
                    ++pos;
                }
            }
            if (indptr) indptr[2 * i + row + 1] = pos;
        }
    }
    if (nnz_out) *nnz_out = pos;
    return PCS_OK;
}

int pcs_set_unfixed(pcs_engine *h, const uint8_t *unfixed, int64_t *nnz_out) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_set_unfixed: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    std::vector<uint32_t> keep(h->det.n);
    std::vector<int64_t> off(h->det.n);
    int64_t pos = 0;
    for (int64_t i = 0; i < h->det.n; ++i) {
        keep[i] = keep_mask(h, unfixed, i);
        off[i] = pos;
        pos += 2 * __builtin_popcount(keep[i]);
    }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(wait_done_host(h));   // an evaluation on any stream may still read the masks
    HIPCHK(hipStreamSynchronize(h->stream));
    if (const int rc = h->d_keep.grow(h->det.n, sizeof(uint32_t))) return rc;   // released with the table: allocated once per table
    if (const int rc = h->d_row_off.grow(h->det.n, sizeof(int64_t))) return rc;
    HIPCHK(hipMemcpy(h->d_keep.p, keep.data(), sizeof(uint32_t) * h->det.n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_row_off.p, off.data(), sizeof(int64_t) * h->det.n, hipMemcpyHostToDevice));
    h->nnz = pos;
    if (nnz_out) *nnz_out = pos;
    return PCS_OK;
}

int pcs_eval_compact_device(pcs_engine *h, const double *param_str, void *d_resid, void *d_data, void *stream) {
    if (!h || !param_str) return fail(PCS_ERR_ARG, "pcs_eval_compact_device: bad arguments");
    if (h->nnz < 0) return fail(PCS_ERR_STATE, "pcs_set_unfixed has not been called");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    HIPCHK(hipSetDevice(h->device));
    int rc = stage_params(h, param_str, s);
    if (rc) return rc;
    return enqueue_eval(h, h->d_param.as<double>(), d_resid, d_data, true, s);
}

int pcs_eval_compact(pcs_engine *h, const double *param_str, double *resid, double *data) {
    if (!h || !param_str) return fail(PCS_ERR_ARG, "pcs_eval_compact: bad arguments");
    if (h->nnz < 0) return fail(PCS_ERR_STATE, "pcs_set_unfixed has not been called");
    int rc = ensure_scratch(h, resid != nullptr, false, data != nullptr);
    if (rc) return rc;
    rc = pcs_eval_compact_device(h, param_str, resid ? h->d_resid.p : nullptr, data ? h->d_data.p : nullptr, nullptr);
    if (rc) return rc;
    if (resid && (rc = download(h, resid, h->d_resid.p, 2 * h->det.n, h->stream))) return rc;
    if (data && h->nnz > 0 && (rc = download(h, data, h->d_data.p, h->nnz, h->stream))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return PCS_OK;
}

int pcs_legacy_cost(pcs_engine *h, const double *im_points, const double *proj, const double *intrinsics, const double *dists,
                    double *errors) {
    if (!h || !im_points || !proj || !intrinsics || !dists || !errors) return fail(PCS_ERR_ARG, "pcs_legacy_cost: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    if (h->chain == PCS_CHAIN_FREE) return fail(PCS_ERR_ARG, "pcs_legacy_cost: needs an engine with images (template or self chain)");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int64_t n_pts = h->n_imgs * h->n_keys * 3;
    if (const int rc = h->d_im_points.grow(n_pts, sizeof(double))) return rc;
    if (const int rc = h->d_cam_tab.grow(h->n_cams * LEGACY_STRIDE, sizeof(double))) return rc;
    int rc = ensure_scratch(h, true, false, false);
    if (rc) return rc;
    std::vector<double> tab((size_t)h->n_cams * LEGACY_STRIDE, 0.0);
    for (int64_t c = 0; c < h->n_cams; ++c) {
        double *t = tab.data() + c * LEGACY_STRIDE;
        for (int j = 0; j < 12; ++j) t[j] = proj[12 * c + j];
        const double *K = intrinsics + 9 * c;
        t[12] = K[0]; t[13] = K[2]; t[14] = K[4]; t[15] = K[5];  // focal_0, centre_0, focal_1, centre_1 (ch:453-454)
        for (int j = 0; j < 5; ++j) t[16 + j] = dists[5 * c + j];
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpyAsync(h->d_im_points.p, im_points, sizeof(double) * n_pts, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->d_cam_tab.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // `tab` is a local
    const int64_t n_tiles = (h->det.n + 63) / 64;
    const dim3 grid((unsigned)std::min<int64_t>((n_tiles + 3) / 4, (int64_t)h->n_cu * 16));
    hipEvent_t *ev = ring_slot(h, false);
    hipExtLaunchKernelGGL(legacy_cost_kernel, grid, dim3(256), 0, s, ev[2], ev[3], 0, h->det.table(), h->d_im_points.as<const double>(),
                          h->d_cam_tab.as<const double>(), h->d_resid.as<double>(), h->det.n, h->n_keys, h->d_sink.p);
    HIPCHK(hipGetLastError());
    ++h->ev_count;
    h->events_valid = true;
    HIPCHK(mark_done(h, s));
    return download(h, errors, h->d_resid.p, 2 * h->det.n, s, sizeof(double));
}

int pcs_linearize(pcs_engine *h, const double *param_str) {
    if (!h || !param_str) return fail(PCS_ERR_ARG, "pcs_linearize: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    if (h->chain == PCS_CHAIN_TEMPLATE && !h->have_template) return fail(PCS_ERR_STATE, "template points not set");
    HIPCHK(hipSetDevice(h->device));
    int rc = stage_params(h, param_str, h->stream);
    if (rc) return rc;
    rc = launch_slab_prep(h, h->d_param.as<double>(), h->stream);
    if (rc) return rc;
    HIPCHK(mark_done(h, h->stream));
    return PCS_OK;
}

int pcs_matfree(pcs_engine *h, int op, const double *in, double *out, double *cost) {
    if (!h || op < OP_JV || op > OP_GRAD || !out) return fail(PCS_ERR_ARG, "pcs_matfree: bad arguments");
    if ((op == OP_JV || op == OP_JTU || op == OP_JTJV) && !in) return fail(PCS_ERR_ARG, "pcs_matfree: this operator needs an input vector");
    if (!h->linearized) return fail(PCS_ERR_STATE, "pcs_matfree: call pcs_linearize (or an evaluation) first");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    HIPCHK(order_after_done(h, s));  // the slabs may have been prepared on a caller stream
    const int64_t n_in = (op == OP_JTU) ? 2 * h->det.n : (op == OP_JV || op == OP_JTJV) ? h->n_params : 0;
    const int64_t n_out = (op == OP_JV) ? 2 * h->det.n : h->n_params;
    if (const int rc = h->d_vin.grow(n_in, sizeof(double))) return rc;
    if (const int rc = h->d_vout.grow(n_out, sizeof(double))) return rc;
    if (const int rc = h->d_cost.grow(1, sizeof(double))) return rc;
    if (n_in) HIPCHK(hipMemcpyAsync(h->d_vin.as<double>(), in, sizeof(double) * n_in, hipMemcpyHostToDevice, s));
    if (op != OP_JV) HIPCHK(hipMemsetAsync(h->d_vout.as<double>(), 0, sizeof(double) * n_out, s));
    if (op == OP_GRAD) HIPCHK(hipMemsetAsync(h->d_cost.as<double>(), 0, sizeof(double), s));
    MatfreeArgs a{};
    a.tab = h->det.table();
    a.cam_slab = h->d_cam_slab.p; a.pose_slab = h->d_pose_slab.p; a.points = h->d_points.p;
    a.vin = h->d_vin.as<double>(); a.vout = h->d_vout.as<double>(); a.cost = h->d_cost.as<double>();
    a.n = h->det.n; a.n_tiles = (h->det.n + TILE - 1) / TILE;
    a.extr_off = h->extr_off; a.pose_off = h->pose_off; a.point_off = h->point_off;
    a.n_params = (int32_t)h->n_params;
    // workgroup-private LDS accumulators (+ one reduction panel per wave) when they fit
    const size_t acc_bytes = sizeof(double) * (size_t)((h->n_params + 1) & ~(int64_t)1);
    const size_t lds_need = acc_bytes + sizeof(double) * (size_t)WAVES_PER_WG * RED_PANEL;
    const bool lds_acc = h->matfree_lds && op != OP_JV && lds_need <= 150 * 1024;
    const size_t lds = lds_acc ? lds_need : 0;
    const int64_t wpc = h->wgs_per_cu > 0 ? h->wgs_per_cu : (op == OP_JV ? 8 : 2);
    const int64_t target_wgs = (int64_t)h->n_cu * wpc;
    int64_t tpw = h->tiles_per_wg > 0 ? h->tiles_per_wg : (a.n_tiles + target_wgs - 1) / target_wgs;   // option tiles_per_wg: tests of the tile pipeline
    tpw = std::max<int64_t>(WAVES_PER_WG, (tpw + WAVES_PER_WG - 1) / WAVES_PER_WG * WAVES_PER_WG);
    a.tiles_per_wg = (int32_t)tpw;
    const dim3 grid((unsigned)((a.n_tiles + tpw - 1) / tpw));
    hipEvent_t *ev = ring_slot(h, false);
    HIPCHK(hipEventRecord(ev[2], s));
    hipError_t e = launch_matfree_t(h->chain, op, lds_acc, a, grid, lds, s);
    if (e != hipSuccess) return fail(PCS_ERR_HIP, "matfree kernel launch failed: %s", hipGetErrorString(e));
    HIPCHK(hipEventRecord(ev[3], s));
    ++h->ev_count;
    h->events_valid = true;
    HIPCHK(mark_done(h, s));
    HIPCHK(hipMemcpyAsync(out, h->d_vout.as<double>(), sizeof(double) * n_out, hipMemcpyDeviceToHost, s));
    if (op == OP_GRAD && cost) HIPCHK(hipMemcpyAsync(cost, h->d_cost.as<double>(), sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return PCS_OK;
}

int pcs_normal_equations_device(pcs_engine *h, const double *param_str, double *d_H, double *d_g, double *d_cost, void *stream) {
    if (!h || !param_str || !d_H || !d_g || !d_cost) return fail(PCS_ERR_ARG, "pcs_normal_equations_device: bad arguments");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    HIPCHK(hipSetDevice(h->device));
    int rc = stage_params(h, param_str, s);
    if (rc) return rc;
    return enqueue_normal(h, h->d_param.as<double>(), d_H, d_g, d_cost, s);
}

int pcs_normal_layout(const pcs_engine *h, int64_t *out5) {
    if (!h || !out5) return fail(PCS_ERR_ARG, "pcs_normal_layout: bad arguments");
    layout_out5(block_layout(h), h->n_params, out5);
    return PCS_OK;
}

int pcs_normal_blocks_device(pcs_engine *h, const double *d_param_str, double *d_packed, void *stream) {
    if (!h || !d_param_str || !d_packed) return fail(PCS_ERR_ARG, "pcs_normal_blocks_device: bad arguments");
    if (reinterpret_cast<uintptr_t>(d_packed) % 16) return fail(PCS_ERR_ARG, "pcs_normal_blocks_device: the packed buffer must be 16-byte aligned");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    double *d_g = d_packed + block_layout(h).h_len();
    return enqueue_normal(h, d_param_str, d_packed, d_g, d_g + h->n_params, s, true);
}

int pcs_prior_add_device(pcs_engine *h, const double *d_param_str, double *d_packed, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_prior_add_device: bad arguments");
    return prior_add_piece("pcs_prior_add_device", h->device, h->prior, block_layout(h), h->n_params, d_param_str, d_packed, stream ? (hipStream_t)stream : h->stream);
}

// The two bound kernels as calls of their own, for a loop the host steers (pcs_solver.inc: bounds_active_piece, bounds_truncate_piece).
int pcs_bounds_active_device(pcs_engine *h, const double *d_ps, const double *d_packed, const uint8_t *d_fixed, uint8_t *d_fixed_eff, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_bounds_active_device: bad arguments");
    return bounds_active_piece("pcs_bounds_active_device", h->device, h->bounds, block_layout(h), h->n_params, d_ps, d_packed, d_fixed, d_fixed_eff, stream ? (hipStream_t)stream : h->stream);
}

int pcs_bounds_truncate_device(pcs_engine *h, const double *d_ps_in, double *d_delta, double *d_ps_out, double *d_alpha, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_bounds_truncate_device: bad arguments");
    return bounds_truncate_piece("pcs_bounds_truncate_device", h->device, h->bounds, h->n_params, d_ps_in, d_delta, d_ps_out, d_alpha, stream ? (hipStream_t)stream : h->stream);
}

int pcs_bounds_active_sel_device(pcs_engine *h, const double *d_ps0, const double *d_ps1, const double *d_packed0, const double *d_packed1, const uint8_t *d_fixed,
                                 uint8_t *d_fixed_eff, const int32_t *d_sel, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_bounds_active_sel_device: bad arguments");
    return bounds_active_sel_piece("pcs_bounds_active_sel_device", h->device, h->bounds, block_layout(h), h->n_params, d_ps0, d_ps1, d_packed0, d_packed1, d_fixed, d_fixed_eff, d_sel,
                                   stream ? (hipStream_t)stream : h->stream);
}

int pcs_bounds_truncate_sel_device(pcs_engine *h, double *d_ps0, double *d_ps1, double *d_delta, double *d_alpha, const int32_t *d_sel, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_bounds_truncate_sel_device: bad arguments");
    return bounds_truncate_sel_piece("pcs_bounds_truncate_sel_device", h->device, h->bounds, h->n_params, d_ps0, d_ps1, d_delta, d_alpha, d_sel, stream ? (hipStream_t)stream : h->stream);
}

// The pieces of a trial for a loop the host steers (pcs_solver.inc: schur_prepare_piece, schur_finish_piece, lm_decide_piece).
int pcs_schur_prepare(pcs_engine *h, double *d_packed, const uint8_t *d_fixed, const double *d_lambda, double *d_linvt, double *d_u,
                      double *d_V, double *d_S, double *d_rhs, double *d_dvec, double *d_gm, int32_t *d_status, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_schur_prepare: bad arguments");
    return schur_prepare_piece("pcs_schur_prepare", h->device, block_layout(h), stream ? (hipStream_t)stream : h->stream, d_packed, d_fixed, d_lambda, d_linvt, d_u, d_V, d_S, d_rhs, d_dvec, d_gm, d_status);
}

int pcs_schur_finish(pcs_engine *h, const double *d_linvt, const double *d_u, const double *d_w, const double *d_xlead, const uint8_t *d_fixed,
                     double *d_delta, const double *d_ps_in, double *d_ps_out, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_schur_finish: bad arguments");
    return schur_finish_piece("pcs_schur_finish", h->device, block_layout(h), stream ? (hipStream_t)stream : h->stream, d_linvt, d_u, d_w, d_xlead, d_fixed, d_delta, d_ps_in, d_ps_out);
}

int pcs_lm_decide(pcs_engine *h, const double *d_cost_old, const double *d_cost_new, const double *d_dvec, const double *d_gm, const double *d_delta,
                  const double *d_ps, const uint8_t *d_fixed, int32_t *d_status, double *d_lambda, double *d_stats, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_lm_decide: bad arguments");
    return lm_decide_piece("pcs_lm_decide", h->device, h->n_params, stream ? (hipStream_t)stream : h->stream, d_cost_old, d_cost_new, d_dvec, d_gm, d_delta, d_ps, d_fixed, d_status, d_lambda, d_stats);
}

int pcs_lm_decide_bounded(pcs_engine *h, const double *d_cost_old, const double *d_cost_new, const double *d_dvec, const double *d_gm, const double *d_delta,
                          const double *d_ps, const uint8_t *d_fixed_eff, const double *d_alpha, int32_t *d_status, double *d_lambda, double *d_stats, void *stream) {
    if (!h || !d_alpha) return fail(PCS_ERR_ARG, "pcs_lm_decide_bounded: bad arguments");
    if (!h->bounds.active()) return fail(PCS_ERR_STATE, "pcs_lm_decide_bounded: no bounds set");
    return lm_decide_piece("pcs_lm_decide_bounded", h->device, h->n_params, stream ? (hipStream_t)stream : h->stream, d_cost_old, d_cost_new, d_dvec, d_gm, d_delta, d_ps, d_fixed_eff, d_status, d_lambda, d_stats, d_alpha, h->bounds.pin());
}

// One Levenberg-Marquardt trial in two halves (pcs_solver.inc: enqueue_lm_trial_build, enqueue_lm_finish).
int pcs_lm_trial_build(pcs_engine *h, const pcs_lm_buffers *b, void *stream) {
    const int rc = lm_check(h, b, "pcs_lm_trial_build");
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    LmTrialDesc d;
    d.who = "pcs_lm_trial_build"; d.device = h->device; d.n_cu = h->n_cu; d.n_params = h->n_params; d.L = block_layout(h);
    d.deterministic = h->deterministic != 0; d.spd_timeout_us = h->spd_timeout_us;
    d.bounds = &h->bounds;
    d.fused = h->fused_trial && d.L.n_lead > 0 && d.L.n_ent > 0 && h->det.n > 0 && !h->bounds.active();
    d.selector = true;
    d.empty_zero_state = h->det.n == 0;
    d.slabs = FinishSlabs{h->d_cam_slab.as<double>(), h->d_pose_slab.as<double>(), h->d_points.as<double>(), h->n_cams, h->n_imgs, h->n_keys, h->extr_off, h->pose_off, h->point_off,
                          h->chain != PCS_CHAIN_FREE, h->chain != PCS_CHAIN_TEMPLATE};
    return enqueue_lm_trial_build(d, b, stream ? (hipStream_t)stream : h->stream, [&](hipStream_t s, bool fused) {
        const int64_t alt_pk = b->packed[1] - b->packed[0], alt_ps = b->ps[1] - b->ps[0];   // doubles from state 0 to state 1
        double *g_new = b->packed[1] + d.L.h_len();
        return enqueue_normal(h, b->ps[1], b->packed[1], g_new, g_new + h->n_params, s, true, NormalTrial{b->flags, b->flags + 2, -alt_ps, -alt_pk, fused});
    });
}

int pcs_lm_trial_finish(pcs_engine *h, const pcs_lm_buffers *b, void *stream) {
    const int rc = lm_check(h, b, "pcs_lm_trial_finish");
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    return enqueue_lm_finish(h->n_cu, h->n_params, block_layout(h), h->prior, h->bounds, b, stream ? (hipStream_t)stream : h->stream);
}

int pcs_lm_trial(pcs_engine *h, const pcs_lm_buffers *b, void *stream) {
    const int rc = pcs_lm_trial_build(h, b, stream);
    return rc ? rc : pcs_lm_trial_finish(h, b, stream);
}

int pcs_normal_equations(pcs_engine *h, const double *param_str, double *H, double *g, double *cost) {
    if (!h || !param_str || !H || !g || !cost) return fail(PCS_ERR_ARG, "pcs_normal_equations: bad arguments");
    if (h->det.n <= 0) return fail(PCS_ERR_STATE, "no detections set");
    if (h->n_params > PCS_NORMAL_MAX_PARAMS)  // the same limit as enqueue_normal, checked BEFORE the scratch allocation
        return fail(PCS_ERR_ARG, "pcs_normal_equations: %lld parameters make a dense J^T J of %.1f GB (limit %d parameters: 32-bit offsets); use pcs_matfree",
                    (long long)h->n_params, (double)h->n_params * (double)h->n_params * 8e-9, PCS_NORMAL_MAX_PARAMS);
    HIPCHK(hipSetDevice(h->device));
    const int64_t need = h->n_params * h->n_params + h->n_params + 1;  // H | g | cost in one scratch buffer
    if (const int rc = h->d_H.grow(need, sizeof(double))) return rc;
    double *d_g = h->d_H.as<double>() + h->n_params * h->n_params, *d_cost = d_g + h->n_params;
    int rc = pcs_normal_equations_device(h, param_str, h->d_H.as<double>(), d_g, d_cost, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(H, h->d_H.as<double>(), sizeof(double) * h->n_params * h->n_params, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(g, d_g, sizeof(double) * h->n_params, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(cost, d_cost, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return PCS_OK;
}

int pcs_synchronize(pcs_engine *h, void *stream) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_synchronize: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(stream ? (hipStream_t)stream : h->stream));
    return PCS_OK;
}

int pcs_last_kernel_ms(pcs_engine *h, float *slab_prep_ms, float *eval_ms) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_last_kernel_ms: bad arguments");
    if (!h->events_valid) return fail(PCS_ERR_STATE, "no evaluation has been queued yet");
    float a = 0, b = 0;
    int rc = ring_read(h, (h->ev_count - 1) % h->ev_ring, &a, &b);
    if (rc) return rc;
    if (slab_prep_ms) *slab_prep_ms = a;
    if (eval_ms) *eval_ms = b;
    return PCS_OK;
}

int pcs_kernel_ms_mean(pcs_engine *h, int64_t *count, float *slab_prep_ms, float *eval_ms) {
    if (!h) return fail(PCS_ERR_ARG, "pcs_kernel_ms_mean: bad arguments");
    if (!h->events_valid) return fail(PCS_ERR_STATE, "no evaluation has been queued yet");
    const int64_t n = std::min<int64_t>(h->ev_count, h->ev_ring);
    double sa = 0, sb = 0;
    for (int64_t i = 0; i < n; ++i) {
        float a = 0, b = 0;
        int rc = ring_read(h, i, &a, &b);
        if (rc) return rc;
        sa += a;
        sb += b;
    }
    if (count) *count = n;
    if (slab_prep_ms) *slab_prep_ms = (float)(sa / n);
    if (eval_ms) *eval_ms = (float)(sb / n);
    return PCS_OK;
}

int pcs_kernel_ms_samples(pcs_engine *h, int64_t capacity, float *slab_prep_ms, float *eval_ms, int64_t *count) {
    if (!h || capacity < 0 || !count || (capacity > 0 && (!slab_prep_ms || !eval_ms))) return fail(PCS_ERR_ARG, "pcs_kernel_ms_samples: bad arguments");
    if (!h->events_valid) return fail(PCS_ERR_STATE, "no evaluation has been queued yet");
    const int64_t have = std::min<int64_t>(h->ev_count, h->ev_ring), n = std::min<int64_t>(have, capacity);
    const int64_t first = h->ev_count - n;   // the n most recent evaluations, oldest first
    for (int64_t i = 0; i < n; ++i) {
        int rc = ring_read(h, (first + i) % h->ev_ring, slab_prep_ms + i, eval_ms + i);
        if (rc) return rc;
    }
    *count = n;
    return PCS_OK;
}

int pcs_normal_descriptors(int chain, int pass, int trail_group, int32_t *out) {
    if (!out || chain < 0 || chain > 2 || pass < 0 || pass > 1 || (pass == PASS_CAMKEY && chain == CHAIN_TEMPLATE))
        return fail(PCS_ERR_ARG, "pcs_normal_descriptors: bad arguments (passes 0 and 1 of ba_normal_mfma_kernel only)");
    if (pass == PASS_SHARED) {
        if (chain == CHAIN_TEMPLATE) fill_descriptors<CHAIN_TEMPLATE, PASS_SHARED>(trail_group, out);
        else if (chain == CHAIN_SELF) fill_descriptors<CHAIN_SELF, PASS_SHARED>(trail_group, out);
        else fill_descriptors<CHAIN_FREE, PASS_SHARED>(trail_group, out);
    } else {
        if (chain == CHAIN_SELF) fill_descriptors<CHAIN_SELF, PASS_CAMKEY>(trail_group, out);
        else fill_descriptors<CHAIN_FREE, PASS_CAMKEY>(trail_group, out);
    }
    return PCS_OK;
}

int pcs_normal_entry_map(int chain, int pass, int32_t *out) {
    if (!out || chain < 0 || chain > 2 || pass < 0 || pass > 2) return fail(PCS_ERR_ARG, "pcs_normal_entry_map: bad arguments");
    if ((pass != PASS_SHARED && chain == CHAIN_TEMPLATE) || (pass == PASS_IMGKEY && chain != CHAIN_SELF))
        return fail(PCS_ERR_ARG, "pcs_normal_entry_map: chain %d has no pass %d", chain, pass);
    if (pass == PASS_SHARED) {
        if (chain == CHAIN_TEMPLATE) fill_entry_map<CHAIN_TEMPLATE, PASS_SHARED>(out);
        else if (chain == CHAIN_SELF) fill_entry_map<CHAIN_SELF, PASS_SHARED>(out);
        else fill_entry_map<CHAIN_FREE, PASS_SHARED>(out);
    } else if (pass == PASS_CAMKEY) {
        if (chain == CHAIN_SELF) fill_entry_map<CHAIN_SELF, PASS_CAMKEY>(out);
        else fill_entry_map<CHAIN_FREE, PASS_CAMKEY>(out);
    } else {
        // ba_normal_imgkey_kernel: register r of lane l = entry (a, b), a <= b, of the run's 3 x 3 sum G = S^T S over the
        // pose-translation columns 18..20 (column l & 15 in the order 00 01 02 11 12 22), for local run (l >> 4) + 4 r
        static const int ga[IK_COLS] = {0, 0, 0, 1, 1, 2}, gb[IK_COLS] = {0, 1, 2, 1, 2, 2};
        for (int m = 0; m < 2; ++m)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r) {
                    const int c = lane & 15;
                    int32_t *o = out + ((m * 64 + lane) * 4 + r) * 2;
                    o[0] = (m == 0 && c < IK_COLS) ? 18 + ga[c] : -1;
                    o[1] = (m == 0 && c < IK_COLS) ? 18 + gb[c] : -1;
                }
    }
    return PCS_OK;
}

}  // extern "C"

#include "pcs_genchain.inc"
