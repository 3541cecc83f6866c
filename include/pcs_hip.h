/*
 * pcs_hip.h — C ABI of the MI355X bundle-adjustment cost/Jacobian engine (libpcs_hip.so).
 *
 * Drop-in boundary for pyCamSet's optimisation hot path.  Every entry point names the
 * reference interface it replaces (paths relative to the reference repo, pyCamSet/optimisation/
 * unless stated: afb = abstract_function_blocks.py, th = template_handler.py,
 * sbh = standard_bundle_handler.py, fph = free_point_handler.py,
 * td = ../calibration_targets/target_detections.py).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types cross the boundary.
 *   - every function returns PCS_OK (0) or a negative pcs_status; pcs_last_error() gives text
 *     for the calling thread's most recent failure.  No exception crosses the ABI.
 *   - the caller owns every buffer it passes; the engine owns its device buffers for the
 *     lifetime of the handle.  One handle = one host thread at a time.
 *   - streams: the *_device entry points take a stream; work a handle queues on different streams is ordered
 *     by the engine (an event recorded after every enqueue is waited for before the shared slabs, the staging
 *     buffer or the masks are touched again), so consecutive calls may use different streams.  What the engine
 *     cannot order is the CALLER's use of the output buffers: synchronise the stream a call was queued on (or
 *     pcs_synchronize) before reading them from another stream or from the host.
 *   - numerical inf/nan (e.g. a point on the camera plane, z = 0) pass through unchanged,
 *     as in the reference's numba code.
 *   - there is NO CPU fallback: without a HIP device pcs_create fails with PCS_ERR_NODEVICE.
 */
#ifndef PCS_HIP_H
#define PCS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pcs_engine pcs_engine;

typedef enum {
    PCS_OK = 0,
    PCS_ERR_ARG = -1,      /* null pointer, bad enum, bad size */
    PCS_ERR_HIP = -2,      /* a HIP runtime call failed (text in pcs_last_error) */
    PCS_ERR_STATE = -3,    /* detections / template / structure not set yet */
    PCS_ERR_NODEVICE = -4, /* no usable HIP device */
    PCS_ERR_RANGE = -5     /* a detection indexes outside [0,n_cams) x [0,n_imgs) x [0,n_keys) */
} pcs_status;

/* Function-block chains (the three `op_fun` sums the reference handlers build). */
typedef enum {
    PCS_CHAIN_TEMPLATE = 0, /* projection + extrinsic3D + template_points          th:152   P = 21 */
    PCS_CHAIN_SELF = 1,     /* projection + extrinsic3D + rigidTform3d + free_point sbh:182  P = 24 */
    PCS_CHAIN_FREE = 2      /* projection + extrinsic3D + free_point                fph:143  P = 18 */
} pcs_chain;

/* Arithmetic and parameter slabs are FP64 for every dtype (the reference's precision, fbi:11); the dtype selects the
 * BYTES of the streams:  PCS_F64   measurements double, residual / Jacobian double   (380 B per detection, chain T)
 *                        PCS_F32   measurements float,  residual / Jacobian float    (196 B) — BASELINE config 5
 *                        PCS_MIXED measurements double, residual / Jacobian float    (204 B)
 * A float output is the FP64 result rounded once at the store (<= 1.2e-7 relative); PCS_F32 additionally rounds the
 * measured (u, v) to float on upload (<= 6e-5 px at ~1e3 px).  Round 1's all-float arithmetic (5e-3 relative error
 * from cancellation in the chain rule) is gone.  Device outputs of the *_device entry points are float for PCS_F32
 * and PCS_MIXED. */
typedef enum { PCS_F64 = 0, PCS_F32 = 1, PCS_MIXED = 2 } pcs_dtype;

/* Library / build identification. */
int pcs_version(void);
const char *pcs_last_error(void);
/* Number of HIP devices visible (0 when none); never fails. */
int pcs_device_count(void);

/*
 * Create an engine for one chain on one device.
 * Replaces: optimisation_function.__init__/_prep_for_computation (afb:111-190) +
 *           make_param_struct (afb:777-820).  The reference derives the group counts from the
 *           detection table (max index + 1, afb:793-795); here they are explicit arguments.
 * Parameter-string layout (same as the reference):
 *   intr 9*c+j | extr 9*C + 6*c+j | pose 15*C + 6*i+j (chains T,S) | point (15*C+6*I | 15*C) + 3*k+j (S | F)
 */
int pcs_create(pcs_engine **out, int chain, int dtype, int64_t n_cams, int64_t n_imgs, int64_t n_keys, int device);
int pcs_destroy(pcs_engine *h);

int64_t pcs_n_params(const pcs_engine *h);     /* length of the full parameter string */
int pcs_row_len(const pcs_engine *h);          /* P: dense Jacobian entries per row */
int64_t pcs_n_detections(const pcs_engine *h); /* N */

/*
 * Upload the static detection table.
 * Replaces: the closure state captured by make_full_loss_template / make_full_jac_template
 *           (_reshape_data_for_parallel afb:281-288, get_block_param_inds afb:192-233).
 * pcs_set_detections_table takes the reference's own (N,5) float64 table
 * [cam, im, key, u, v] (td:51-55 after return_flattened_keys td:333-351); indices are cast with
 * (int) like afb:214 / afb:375.  pcs_set_detections takes the split form.
 * Indices are range-checked against the counts given to pcs_create -> PCS_ERR_RANGE.
 */
int pcs_set_detections_table(pcs_engine *h, const double *det5, int64_t n);
int pcs_set_detections(pcs_engine *h, const int32_t *cam, const int32_t *img, const int32_t *key,
                       const double *uv /* n x 2 */, int64_t n);

/*
 * Upload the constant template points (chain TEMPLATE only), (n_keys, 3) float64.
 * Replaces: the `template` argument of the generated loss/jac (afb:352-354, afb:374-375;
 *           th:160, th:174 `target.point_data.reshape((-1, 3))`).
 */
int pcs_set_template(pcs_engine *h, const double *points);

/*
 * One evaluation at a full parameter string (host buffers, synchronous).
 * Replaces: generated full_loss (afb:350-387) and full_jac (afb:552-599) + the [:n_elements]
 *           truncation (afb:641).
 *   resid : (N,2) row-major  = projected - measured            (afb:384) or NULL
 *   jac   : (2N,P) row-major dense block rows, u row then v row (afb:591-594) or NULL
 * Both are float64 on the host whatever the engine dtype (an F32 engine computes and stores
 * float32 on the device and widens on the way out).
 */
int pcs_eval(pcs_engine *h, const double *param_str, double *resid, double *jac);

/*
 * Same evaluation, asynchronous, outputs left in device memory (engine dtype), launched on
 * `stream` (a hipStream_t passed as void*, NULL = the engine's own non-blocking stream; to queue on the
 * process's default (NULL) stream pass hipStreamLegacy, i.e. (hipStream_t)1 — work on the engine stream is
 * NOT ordered against the default stream).
 *   d_resid : device pointer, N*2 elements, or NULL
 *   d_jac   : device pointer, 2N*P elements, or NULL
 * param_str is a host pointer (copied through a pinned staging buffer); use
 * pcs_eval_device_resident when the parameter string already lives on the device.
 */
int pcs_eval_device(pcs_engine *h, const double *param_str, void *d_resid, void *d_jac, void *stream);
int pcs_eval_device_resident(pcs_engine *h, const double *d_param_str, void *d_resid, void *d_jac, void *stream);

/*
 * Static CSR structure for a given fixed-parameter mask.
 * Replaces: make_jac_CSR_columns_row_pointers (afb:465-489).
 *   unfixed : n_params bytes (non-zero = free), NULL = all free
 *   indices : nnz int64 (pass NULL to only query nnz), indptr : 2N+1 int64 (may be NULL)
 */
int pcs_csr_structure(pcs_engine *h, const uint8_t *unfixed, int64_t *indices, int64_t *indptr, int64_t *nnz);
/* Per-detection global column table (N,P) int64.  Replaces: get_block_param_inds(unthreaded) afb:192-233. */
int pcs_block_param_inds(pcs_engine *h, int64_t *out);

/*
 * Fixed-parameter compaction on the device.
 * Replaces: `data[:n_elements][good_mask]` (afb:627-651) — the reference's per-call host
 * boolean-mask copy.  pcs_set_unfixed prepares the static per-row offsets; pcs_eval_compact
 * writes only the unfixed entries, in CSR data order.
 */
int pcs_set_unfixed(pcs_engine *h, const uint8_t *unfixed, int64_t *nnz);
int pcs_eval_compact(pcs_engine *h, const double *param_str, double *resid, double *data /* nnz */);
int pcs_eval_compact_device(pcs_engine *h, const double *param_str, void *d_resid, void *d_data, void *stream);

/*
 * Matrix-free products with the Jacobian at a linearisation point: J is never
 * materialised.  Replaces what scipy does with the reference's CSR Jacobian
 * (optimisation_handling.py:88-98: x_scale='jac' column norms, J^T f, lsmr mat-vecs).
 * pcs_linearize prepares the slabs at `param_str` (so does a pcs_eval* call that launched slab_prep — not a one-launch step,
 * option "fuse_prep": pcs_matfree then returns PCS_ERR_STATE until pcs_linearize has run).
 * pcs_matfree ops (vectors on the host, FULL parameter-string space, float64):
 *   0 JV    in: n_params            out: 2N        out = J in
 *   1 JTU   in: 2N                  out: n_params  out = J^T in
 *   2 JTJV  in: n_params            out: n_params  out = J^T (J in)
 *   3 DIAG  in: NULL                out: n_params  out = diag(J^T J)
 *   4 GRAD  in: NULL                out: n_params  out = J^T r,  *cost = sum r^2 (cost may be NULL)
 * Sums use f64 atomics: their last bits depend on arrival order.
 */
int pcs_linearize(pcs_engine *h, const double *param_str);
int pcs_matfree(pcs_engine *h, int op, const double *in, double *out, double *cost);

/* Block-reduced normal equations at param_str (what a Levenberg-Marquardt step needs
 * from the Jacobian that optimisation_handling.py:88-98 hands to scipy), built in one pass without
 * writing J:  H = J^T J  (n_params x n_params row-major, FULL parameter-string space, only the UPPER
 * triangle incl. the diagonal is written, the rest is zero),  g = J^T r  (n_params),  cost = r^T r.
 * float64 whatever the engine dtype.  The sums use f64 atomics: the last bits depend on arrival order.  The kernels address H
 * with 32-bit offsets in doubles: n_params <= PCS_NORMAL_MAX_PARAMS = 65535 (a 34 GB matrix; 23170 until round 4); both entry points return
 * PCS_ERR_ARG beyond it, before anything is allocated.
 *   pcs_normal_equations         host buffers (engine-owned device scratch, blocking)
 *   pcs_normal_equations_device  device buffers of the caller, queued on `stream` (NULL = engine stream);
 *                                the call zeroes them first.  Observation shards: all-reduce H, g, cost. */
#define PCS_NORMAL_MAX_PARAMS 65535
int pcs_normal_equations(pcs_engine *h, const double *param_str, double *H, double *g, double *cost);
int pcs_normal_equations_device(pcs_engine *h, const double *param_str, double *d_H, double *d_g, double *d_cost, void *stream);

/* The same normal equations in BLOCKED form, for a solver that stays on the device (round 3): the parameter string splits
 * into a leading part (cameras; + poses for the self chain) and the trailing group whose entities never share a detection
 * (poses of the template chain — 6 columns each —, points of the self / free chains — 3 each), and only what is structurally
 * non-zero is stored:
 *     d_packed = [ A (n_lead x n_lead, upper triangle) | B (n_lead x n_trail) | C (n_trail / tb blocks of tb x tb, upper
 *                  triangle) | g (n_params) | cost (1) ]     float64, 16-byte aligned, zeroed by the call.
 * pcs_normal_layout: out5 = {n_lead, n_trail, tb, length of d_packed in doubles, n_params}.  The parameter string is read
 * from DEVICE memory (d_param_str), so an LM loop never stages it through the host.  Limits: each region below 2^32 doubles (32 GiB).
 * Observation shards: all-reduce d_packed.  Consumer: pycamset_amd/device_solver.py (reference consumer of J:
 * optimisation_handling.py:88-98). */
int pcs_normal_layout(const pcs_engine *h, int64_t *out5);
int pcs_normal_blocks_device(pcs_engine *h, const double *d_param_str, double *d_packed, void *stream);
/* The block-shaped parts of one damped step (H + lambda diag(H)) x = -g on the packed form (csrc/ba_schur.hpp; all pointers
 * are device memory, lambda included):
 *   pcs_schur_prepare  per trailing entity C_e + lambda D_e = L L' -> d_linvt (n_ent x tb x tb: L^-T), d_u (n_trail: L^-1 g_e);
 *                      d_V (n_lead x n_trail) = B L^-T;  d_S (n_lead x n_lead) = sym(A) + lambda D;  d_rhs = -g_lead;
 *                      d_dvec (n_params) = D;  d_gm (n_params) = g.  Parameters with d_fixed[i] != 0 (n_params bytes) get identity
 *                      rows / columns and a zero gradient (B is masked in place).  *d_status |= 1 when a trailing block is
 *                      not positive definite.  The caller then forms S -= V V', rhs += V u, solves S x_l = rhs (library
 *                      GEMM / Cholesky) and w = V' x_l, and
 *   pcs_schur_finish   writes the step in parameter-string order: d_delta (n_params) = [x_l | -L^-T (u + w)], 0 where fixed; with
 *                      d_ps_in / d_ps_out (both or neither) also the trial parameter string d_ps_out = d_ps_in + d_delta.
 *   pcs_lm_decide      the accept / reject decision of the trial on the device: predicted reduction 0.5 (lambda d'D d - g'd), actual
 *                      reduction 0.5 (cost_old - cost_new), gain ratio, *d_lambda <- the next damping (x 1/3 | 1 | 2 by the ratio, x 4
 *                      on a rejected or failed step), *d_status <- 0, and d_stats[12] = {accepted (-1: bit 2 of *d_status was set — the dense solve
 *                      did not complete, the trial is void), max |g|, relative cost drop, |step|,
 *                      |x| over the free parameters, new sum r^2, old sum r^2, lambda used, 0, 0, 0, the next lambda} — the one vector the host reads per trial
 *                      ([8] .. [10] are the stop code, the trial number and the current state of the device-steered loop, pcs_lm_trial).
 *                      With a prior (pcs_set_prior) added to both states, "sum r^2" in [5] and [6] is the augmented sum, prior term included. */
int pcs_schur_prepare(pcs_engine *h, double *d_packed, const uint8_t *d_fixed, const double *d_lambda, double *d_linvt, double *d_u,
                      double *d_V, double *d_S, double *d_rhs, double *d_dvec, double *d_gm, int32_t *d_status, void *stream);
int pcs_schur_finish(pcs_engine *h, const double *d_linvt, const double *d_u, const double *d_w, const double *d_xlead, const uint8_t *d_fixed,
                     double *d_delta, const double *d_ps_in, double *d_ps_out, void *stream);
int pcs_lm_decide(pcs_engine *h, const double *d_cost_old, const double *d_cost_new, const double *d_dvec, const double *d_gm, const double *d_delta,
                  const double *d_ps, const uint8_t *d_fixed, int32_t *d_status, double *d_lambda, double *d_stats, void *stream);

/* One whole LM trial per call — the device-steered form of the loop optimisation_handling.py:88-98 leaves to scipy.
 * The loop keeps TWO states (packed normal equations + parameter string each); flags[2] names the current one, the other receives the
 * trial.  pcs_lm_trial_build queues, on `stream`: the damped Schur step from the current state at *lambda (pcs_schur_prepare,
 * pcs_schur_syrk, pcs_dense_spd_solve_algo, pcs_schur_vtx, pcs_schur_finish: delta and the trial string = current string + delta) and
 * the blocked normal equations at the trial string into the trial state.  pcs_lm_trial_finish queues the decision (pcs_lm_decide's
 * arithmetic + the loop's termination rules from `ctrl`), which makes an accepted trial the current state by flipping flags[2] (no
 * copy), and writes the 12-double read-back into stats_host (page-locked; may be NULL).  pcs_lm_trial = both.  A loop over observation
 * shards (one process per GPU) queues its all-reduce of the trial state BETWEEN the two halves, on the same stream (RCCL: stream-
 * ordered, no host synchronisation); because that collective is queued on a fixed address, such a loop sets
 * PCS_LM_FIXED_TRIAL_BUFFER: state 0 stays current, trials are built into state 1 and an accepted one is copied over state 0.
 * Every kernel of the sequence first reads flags[0] and does nothing when it is set, so a caller may queue the NEXT trial before it has
 * seen this one's verdict: the GPU never waits for the host between trials.
 *   ctrl (12 doubles, device): [0] stop code, 0 = running (1 gtol reached before the step, 2 `ctrl[7]` consecutive rejections, 3 ftol,
 *        4 xtol, 5 `ctrl[3]` accepted steps, 9 the one-launch dense solve gave up — set spd_algorithm = PCS_SPD_LAUNCHES, clear ctrl[0] and
 *        flags[0] and queue the trial again), [1] consecutive rejections, [2] accepted steps, [3] iteration limit, [4] ftol, [5] xtol,
 *        [6] gtol, [7] rejection limit, [8] trials decided, [9] the factor a rejection applies to lambda before the first accepted step
 *        (0 = 4, as after it), [10], [11] a gain ratio above ctrl[10] multiplies lambda by ctrl[11] instead of 1/3 (0 = off)
 *   stats (12 doubles, device): pcs_lm_decide's eight, [8] the stop code after this trial, [9] the trial's number (ctrl[8]) or -1 for a
 *        launch that found the flag raised (nothing was computed; everything else in `stats` is then stale), [10] the current state
 *        after this trial (0 / 1), [11] lambda for the next trial.
 *   PCS_LM_VOTES: every rank writes "my dense solve gave up" (0 / 1) into the word behind the trial state's packed buffer (hence
 *        pcs_normal_layout's length + 1), the loop's all-reduce sums it with the blocks, and the decision voids the trial on EVERY
 *        rank when the sum is positive — the ranks repeat it together.
 * All pointers are device memory except stats_host / result_host; sizes as for the entry points named above.  After the loop has ended
 * the buffers may only be touched on `stream` (the speculative trial behind the end is still draining). */
#define PCS_LM_FIXED_TRIAL_BUFFER 1
#define PCS_LM_VOTES 2
typedef struct pcs_lm_buffers {
    double *packed[2];                    /* the two states: [A | B | C | g | cost | votes] (pcs_normal_layout's length + 1), 16-byte aligned */
    double *ps[2];                        /* their parameter strings, n_params each */
    int32_t *flags;                       /* 4 words: [0] stop, [1] the last trial was accepted, [2] the current state, [3] unused */
    const uint8_t *fixed;
    double *lambda;
    double *linvt, *u, *V, *S, *rhs, *dvec, *gm;   /* pcs_schur_prepare's outputs */
    int32_t *status;
    double *xlead, *w, *spd_work;         /* n_lead | n_trail | pcs_dense_spd_work_len(n_lead) */
    double *delta;                        /* n_params */
    double *ctrl;
    double *stats;
    double *stats_host;
    int32_t spd_algorithm;                /* PCS_SPD_* */
    int32_t mode;                         /* PCS_LM_* bits */
    /* optional: when the loop ends with this trial (stop code != 0), the final state — gradient and parameters at the n_free indices
     * free_idx (device, int64), then sum r^2 — goes to result_host (page-locked, mapped; 2 n_free + 1 doubles) BEFORE the read-back of
     * the trial: a host that polls stats_host[9] needs no further copy and no synchronisation to return the solution */
    const int64_t *free_idx;
    int64_t n_free;
    double *result_host;
    /* engine option "deterministic": workspace of the ordered S -= V V' (pcs_schur_syrk_work_len(n_lead, n_trail) doubles; may be NULL
     * when that is 0) */
    double *syrk_work;
    int64_t syrk_work_len;
} pcs_lm_buffers;
int pcs_lm_trial_build(pcs_engine *h, const pcs_lm_buffers *b, void *stream);
int pcs_lm_trial_finish(pcs_engine *h, const pcs_lm_buffers *b, void *stream);
int pcs_lm_trial(pcs_engine *h, const pcs_lm_buffers *b, void *stream);

/* The two products of the Schur step around the dense solve, on raw device pointers (float64, row-major):
 *   pcs_schur_syrk   S -= V V' on the LOWER triangle of S (n_lead x n_lead, row stride lds; V n_lead x n_trail, row stride ldv) and,
 *                    when d_u is given, rhs += V u — FP64 matrix cores, one workgroup per 32 x 32 tile and K split
 *                    (csrc/ba_schur.hpp); the partial sums of a split meet in f64 atomics (last bits run-to-run dependent);
 *   pcs_schur_vtx    w = V' x (n_trail outputs).
 * They replace the rocBLAS GEMM / GEMV calls of the reference consumer's step (optimisation_handling.py:88-98) in the device LM
 * loop; queued on `stream` (NULL = the default stream). */
int pcs_schur_syrk(int device, int64_t n_lead, int64_t n_trail, const double *d_V, int64_t ldv, double *d_S, int64_t lds, const double *d_u,
                   double *d_rhs, void *stream);
int pcs_schur_vtx(int device, int64_t n_lead, int64_t n_trail, const double *d_V, int64_t ldv, const double *d_x, double *d_w, void *stream);
/* pcs_schur_syrk with an ORDER: the partial products of a K split are stored to d_work (pcs_schur_syrk_work_len(n_lead, n_trail) doubles;
 * 0 = this size is not split and d_work is not touched) and subtracted split by split by a second kernel — the same bits on every run
 * and on every rank of a sharded solve (the reference's consumer is deterministic: scipy on one thread, optimisation_handling.py:88-98).
 * What engine option "deterministic" makes pcs_lm_trial_build use. */
int64_t pcs_schur_syrk_work_len(int64_t n_lead, int64_t n_trail);
int pcs_schur_syrk_ordered(int device, int64_t n_lead, int64_t n_trail, const double *d_V, int64_t ldv, double *d_S, int64_t lds, const double *d_u,
                           double *d_rhs, double *d_work, int64_t work_doubles, void *stream);

/* S x = rhs for a dense symmetric positive definite S (float64, n x n row-major with row stride ld, LOWER triangle read and
 * overwritten by its Cholesky factor): the reduced system of the Schur step above — what optimisation_handling.py:88-98 leaves to
 * scipy's trf / lsmr on the host.  Two forms of the same blocked factorisation (32 x 32 tiles):
 *   PCS_SPD_ONE_LAUNCH  one persistent launch (csrc/ba_chol_persist.hpp): every tile lives in the LDS of one workgroup for the whole
 *                       launch, block columns are handed over through HBM (write-through stores + one counter per column), the
 *                       right-hand side rides along as one more block row, the backward substitution is a chain of 32-word hand-offs
 *                       between the owners of the diagonal tiles.  n <= 1 984 on a 256-CU part (8 tiles per workgroup);
 *   PCS_SPD_LAUNCHES    one launch per block column + substitution launches (csrc/ba_dense_chol.hpp): any n <= 32 768;
 *   PCS_SPD_AUTO        the first where it fits.
 * All pointers are device memory; d_work holds pcs_dense_spd_work_len(n) doubles; *d_status |= 2 when a pivot is not positive,
 * |= 4 when the one-launch form gave up waiting (another process holds the compute units: the results are not valid — solve
 * again with PCS_SPD_LAUNCHES); queued on `stream` (NULL = the default stream). */
#define PCS_SPD_AUTO 0
#define PCS_SPD_LAUNCHES 1
#define PCS_SPD_ONE_LAUNCH 2
int64_t pcs_dense_spd_work_len(int64_t n);
int pcs_dense_spd_solve_algo(int device, int64_t n, double *d_S, int64_t ld, const double *d_rhs, double *d_x, double *d_work, int32_t *d_status, void *stream,
                             int algorithm);
int pcs_dense_spd_solve(int device, int64_t n, double *d_S, int64_t ld, const double *d_rhs, double *d_x, double *d_work, int32_t *d_status, void *stream);
/* The same with the one-launch form's time limit spelled out: every wait of a workgroup for a hand-over gives up after timeout_us
 * microseconds (1 .. 60 000 000; the other entry points use 250 000), sets bit 2 of *d_status and lets the whole grid drain.  Inside an LM
 * trial (pcs_lm_trial*) the limit is the engine option "spd_timeout_us".  A caller that sees bit 2 repeats the solve with
 * PCS_SPD_LAUNCHES on the ORIGINAL matrix (the abandoned launch has overwritten part of the lower triangle). */
int pcs_dense_spd_solve_opts(int device, int64_t n, double *d_S, int64_t ld, const double *d_rhs, double *d_x, double *d_work, int32_t *d_status, void *stream,
                             int algorithm, int64_t timeout_us);

/* Parameter covariance from the factor the solve above leaves in S (csrc/ba_covariance.hpp; version 102).  All pointers are device
 * memory, queued on `stream` (NULL = the default stream); bad sizes or NULL pointers return PCS_ERR_ARG without touching the GPU.
 *   pcs_cov_trsm        X <- L^-1 X in place, L = the LOWER triangle of d_L (n x n, row stride ldl; nothing above the diagonal is
 *                       read), X = d_X (n x n_rhs, row stride ldx: V's layout).  flags PCS_COV_TRSM_IDENTITY: X is not read and
 *                       becomes L^-1 (n_rhs = n), its zero upper part written too.  n <= 32 768.
 *   pcs_cov_block_gram  for every block b < n_blocks: the w x w Gram matrix G_b = X[r0:, c : c + w]' X[r0:, c : c + w] of the
 *                       n_rows x n_cols matrix d_X (row stride ldx), c = d_col[b], w = d_width[b] (1 .. 16), r0 = d_row0[b] (NULL: 0),
 *                       written row-major to d_out + b * out_stride (d_out holds (n_blocks - 1) * out_stride + w^2 doubles); a block
 *                       whose columns or rows leave X is written as NaN.  Finish options: with d_linvt (n_ent x tb x tb, L_e^-T as
 *                       pcs_schur_prepare leaves it) block b is entity c / tb and becomes L_e^-T (I + G_b) L_e^-1 (w must be tb and
 *                       c a multiple of tb); the result is multiplied by scale (times *d_scale when d_scale is not NULL); with
 *                       d_fixed the rows and columns of parameters d_fixed[fixed_off + column] != 0 are set to exactly 0.  The
 *                       result is symmetric; every sum is taken in a fixed order (no atomics): two calls return the same bits. */
#define PCS_COV_TRSM_IDENTITY 1
int pcs_cov_trsm(int device, int64_t n, const double *d_L, int64_t ldl, double *d_X, int64_t n_rhs, int64_t ldx, int flags, void *stream);
int pcs_cov_block_gram(int device, const double *d_X, int64_t ldx, int64_t n_rows, int64_t n_cols, const int32_t *d_col, const int32_t *d_width,
                       const int32_t *d_row0, int64_t n_blocks, double *d_out, int64_t out_stride, const double *d_linvt, int64_t tb,
                       const uint8_t *d_fixed, int64_t fixed_off, const double *d_scale, double scale, void *stream);

/* Which entry of H / g / cost every accumulator register of the normal-equations kernel stands for (host function, no
 * GPU needed): out[m][lane][r][2], m < 2 MFMAs, lane < 64, r < 4 registers = the two local column ids (index into
 * a J row, 30 = the residual column) of D_m[(lane >> 4) + 4 r][lane & 15], or -1, -1 where the register is not owned.
 * pass 0 = shared (camera + pose + residual), 1 = (cam, key) point pass, 2 = (image, key) point pass.  Pass 2 is a
 * segmented sum in matrix form: its registers hold, for 16 runs at a time, the symmetric 3 x 3 sum over the
 * pose-translation columns (local ids 18..20) from which the run's pose-point block is finished; register r of lane l
 * belongs to local run (l >> 4) + 4 r.
 * Diagnostic aid: tests/test_host_logic.py checks that every needed column pair is owned exactly once. */
int pcs_normal_entry_map(int chain, int pass, int32_t *out);
/* The packed destination descriptor of every accumulator register of ba_normal_mfma_kernel (passes 0 and 1; host function, no
 * GPU needed): out[m][lane][r], layout documented at entry_descriptor (csrc/ba_normal.hpp).  trail_group = 2 (pose) / 3 (point)
 * for the blocked layout, -1 for the dense one.  tests/test_host_logic.py decodes them for sample runs exactly like the
 * kernel's flush does and checks every owned entry's address against the column pair pcs_normal_entry_map reports. */
int pcs_normal_descriptors(int chain, int pass, int trail_group, int32_t *out);

/*
 * Generated chains.  The reference composes ANY list of function blocks (afb:735-748) and code-generates the loss / Jacobian /
 * chain rule for it (afb:290-419, afb:492-652, mm:147-263); user-written blocks are its extension point (afb:689-775).
 * pycamset_amd/chain_compiler.py does the same for the GPU: for a composition
 *     [projection | user block with 2 outputs] + {rigidTform3d | extrinsic3D | user block}* + [template_points | free_point | user source]
 * it emits the straight-line evaluation of one detection (the user blocks' device bodies pasted in), has hipcc compile it with
 * csrc/ba_generic.hpp for gfx950 and hands the code object to pcs_genchain_create.
 *   code_object_path   .hsaco with the entry points pcs_genchain_prep / pcs_genchain_eval_{1,2,3}[_f32] / pcs_genchain_compact_{2,3}[_f32]
 *   row_len = P (sum of the blocks' parameter counts, <= 64), uses_template: the source is template_points
 *   rigid parameter groups (one Rodrigues slab each): first parameter-string column and entity count per group;
 *   user_off[u]: first column of the parameter group of user block u; intr_off / point_off: projection / free_point groups
 *   (which group and which index — camera / image / key — every block reads is compiled into the code object)
 *   dtype: PCS_F64 | PCS_F32 | PCS_MIXED as for pcs_create (FP64 arithmetic, float streams)
 * Outputs and layouts as pcs_eval: resid (N, 2), jac (2N, P) dense block rows, u row then v row, elements of the handle's dtype.
 * pcs_genchain_set_unfixed + pcs_genchain_eval_compact[_device] write only the unfixed columns, in CSR data order, at the store
 * (`data[:n][good_mask]`, afb:644-651, never exists as a dense array): keep[i] bit j = local column j of detection i is free,
 * row_off[i] = offset of its u row in the data array.
 */
/*
 * The device Jacobian check of ONE user block (abstract_function_block.test_self, the reference's test_self of afb:750-775):
 * pycamset_amd/chain_compiler.py compiles the block's device bodies with csrc/ba_blockcheck.hpp into code_object_path.  points:
 * m rows of [params(np), inp(nin, or the 3 template coordinates when templated)].  Per point: fun_out (nout), jac_out
 * (nout x (np + nin), compute_jac's layout) and fd_out (same layout: fourth-order central differences of fun with step
 * eps^(1/5) max(1, |x_j|); template coordinates are not differentiated).  Synchronous, host buffers; PCS_ERR_ARG when the code
 * object was built for another shape.  Since pcs_version() 103.
 */
int pcs_blockcheck(const char *code_object_path, int device, int np, int nin, int nout, int templated, const double *points, int64_t m,
                   double *fun_out, double *jac_out, double *fd_out);

typedef struct pcs_genchain pcs_genchain;
int pcs_genchain_create(pcs_genchain **out, const char *code_object_path, int row_len, int uses_template, int n_groups, const int64_t *group_off,
                     const int32_t *group_count, int n_user, const int64_t *user_off, int64_t intr_off, int64_t point_off, int64_t n_params, int64_t n_cams,
                     int64_t n_imgs, int64_t n_keys, int dtype, int device);
int pcs_genchain_destroy(pcs_genchain *h);
int pcs_genchain_row_len(const pcs_genchain *h);
int pcs_genchain_set_detections_table(pcs_genchain *h, const double *det5, int64_t n);
int pcs_genchain_set_template(pcs_genchain *h, const double *points);
int pcs_genchain_eval(pcs_genchain *h, const double *param_str, void *resid, void *jac);
int pcs_genchain_eval_device(pcs_genchain *h, const double *d_param_str, void *d_resid, void *d_jac, void *stream);
/* A step of a generated chain is ONE launch (the default, like pcs_eval's fused kernel: every wave prepares the Rodrigues slabs of its
 * tile's (camera, image) pairs itself); on = 0 puts the slab preparation in a launch of its own in front.  Same bits either way. */
int pcs_genchain_set_one_launch(pcs_genchain *h, int on);
int pcs_genchain_set_unfixed(pcs_genchain *h, const uint64_t *keep, const int64_t *row_off, int64_t nnz);
int pcs_genchain_eval_compact(pcs_genchain *h, const double *param_str, void *resid, void *data);
int pcs_genchain_eval_compact_device(pcs_genchain *h, const double *d_param_str, void *d_resid, void *d_data, void *stream);
/* Products with the chain's Jacobian kept on the device — what a solver needs from J (optimisation_handling.py:88-98: column norms,
 * J^T f, mat-vecs), for ANY generated chain: pcs_genchain_linearize writes residual + dense block rows at param_str into the
 * handle's buffers (PCS_F64 chains), pcs_genchain_matfree applies them (csrc/ba_blockrow.hpp) with the op codes and vector shapes
 * of pcs_matfree.  pcs_genchain_set_blocks (once, after create) tells which global column a local column stands for: block b
 * covers local columns [col0_b, col0_b + np_b), its parameters of entity e (link_b: 0 camera, 1 image, 2 key) start at start_b + np_b e. */
int pcs_genchain_set_blocks(pcs_genchain *h, int n_blocks, const int32_t *col0, const int32_t *n_params, const int32_t *link, const int64_t *start);
/* SHARED parameter groups (since pcs_version() 111): a chain compiled with groups that are indexed through a table — one lens for
 * several cameras, image i with the pose of position i mod n, one transform per face of a target, one global parameter set
 * (pycamset_amd.function_blocks.param_type's mod_function / key_type.SINGLE) — takes the tables here: per block of the chain
 * (n_blocks, link as for pcs_genchain_set_blocks) tables[b] = NULL for a block indexed by its entity, else table_len[b] group
 * indices, one per camera / image / key, each in [0, n_mapped[b]); the block's group then holds n_mapped[b] parameter sets and a
 * rigid group must have been created with group_count = n_mapped[b].  Call it once, after create and BEFORE pcs_genchain_set_blocks
 * (whose range check then counts groups) and before the first evaluation.  Nothing is launched.  PCS_ERR_ARG: a table_len that
 * is not the entity count of the link, a call after pcs_genchain_set_blocks or after an evaluation; PCS_ERR_RANGE: a table value
 * outside [0, n_mapped[b]).  The ordered sums (option "deterministic") are refused for such a handle; a shared group is never the
 * trailing group of the blocked normal equations. */
int pcs_genchain_set_group_maps(pcs_genchain *h, int n_blocks, const int32_t *link, const int32_t *const *tables, const int64_t *table_len,
                                const int32_t *n_mapped);
int pcs_genchain_linearize(pcs_genchain *h, const double *param_str);
int pcs_genchain_matfree(pcs_genchain *h, int op, const double *in, double *out, double *cost);
/* The exact Levenberg-Marquardt step for ANY generated chain (round 5; csrc/ba_blockgram.hpp).  Replaces what scipy's trf does with the
 * CSR Jacobian of a composed chain (optimisation_handling.py:88-98) for chains the three hand-fused engines do not cover — user blocks
 * included.  The packed state is pcs_normal_layout's [A | B | C | g | cost] (pcs_genchain_normal_layout: same out5).  A chain whose LAST
 * parameter group is one rigid transform per image (6) or one point per key (3) has that group as the trailing entities — B and the
 * tb x tb blocks of C are filled, the dense factorisation is of the leading part only (Schur step, like the hand-fused chains); every
 * other chain, and any chain after pcs_genchain_set_option("dense_normal", 1), has every parameter leading: A = J^T J DENSE
 * (n_params x n_params, upper triangle written), out5 = {n_params, 0, 3, n_params^2 + n_params + 1, n_params}.
 * pcs_genchain_normal_blocks_device evaluates the chain at d_param_str (block rows into the handle's buffers) and contracts them on the
 * FP64 matrix cores.  pcs_genchain_lm_trial_build / _finish / pcs_genchain_lm_trial are pcs_lm_trial_build / _finish / pcs_lm_trial for
 * the handle (same pcs_lm_buffers, sized from pcs_genchain_normal_layout like pcs_normal_layout's — in the dense form V, linvt, u and w hold
 * one double each —, same decision, read-back and stop word); mode must hold
 * PCS_LM_FIXED_TRIAL_BUFFER (the generated kernel reads its string from a fixed address: the trial is built at ps[1] into packed[1],
 * an accepted one is copied over state 0).  Limits: FP64 chains, row length <= 63, n_params <= PCS_NORMAL_MAX_PARAMS.
 * Options (pcs_genchain_set_option): "spd_timeout_us" (as pcs_set_option), "timing" (0: no start / stop events around evaluations),
 * "dense_normal" (above; changes the layout: set it before buffers are sized), "deterministic" (1: the ORDERED contraction — every
 * segment's matrix to a workspace, groups of consecutive segments added in table order, the K split of schur_syrk through
 * pcs_lm_buffers.syrk_work: the same bits on every run; refused for chains whose blocks share a parameter group),
 * "gram_debug" (measurements only). */
int pcs_genchain_normal_layout(const pcs_genchain *h, int64_t *out5);
int pcs_genchain_normal_blocks_device(pcs_genchain *h, const double *d_param_str, double *d_packed, void *stream);
int pcs_genchain_lm_trial_build(pcs_genchain *h, const pcs_lm_buffers *b, void *stream);
int pcs_genchain_lm_trial_finish(pcs_genchain *h, const pcs_lm_buffers *b, void *stream);
/* The Gaussian parameter prior of a generated chain (since pcs_version() 114): pcs_set_prior / pcs_get_prior / pcs_prior_add_device with
 * the same rules, the same store and the same kernels.  The packed state is the one pcs_genchain_normal_layout describes at the time of
 * the call, so a change of option "dense_normal" is followed (dense: the diagonal entry of every parameter is A[i, i]).
 * pcs_genchain_normal_blocks_device stays the raw sum over the detections; pcs_genchain_lm_trial_finish adds the prior to the trial state. */
int pcs_genchain_set_prior(pcs_genchain *h, const double *mean, const double *inv_sigma, int64_t n);
int pcs_genchain_get_prior(pcs_genchain *h, double *mean, double *inv_sigma, int64_t capacity, int64_t *n);
int pcs_genchain_prior_add_device(pcs_genchain *h, const double *d_param_str, double *d_packed, void *stream);

/* The box bounds of a generated chain (since pcs_version() 118): pcs_set_bounds and its companions with the same meaning, the same store
 * and the same kernels.  pcs_genchain_lm_trial_build consults them (a bounded trial takes the non-fused sequence), and
 * pcs_genchain_lm_trial_finish decides on the truncated step. */
int pcs_genchain_set_bounds(pcs_genchain *h, const double *lo, const double *hi, int64_t n);
int pcs_genchain_get_bounds(pcs_genchain *h, double *lo, double *hi, int64_t capacity, int64_t *n);
int pcs_genchain_bounds_trials(pcs_genchain *h, double *alpha_active, int64_t n_trials, int64_t *n_truncated);
int pcs_genchain_bounds_active_device(pcs_genchain *h, const double *d_ps, const double *d_packed, const uint8_t *d_fixed, uint8_t *d_fixed_eff, void *stream);
int pcs_genchain_bounds_truncate_device(pcs_genchain *h, const double *d_ps_in, double *d_delta, double *d_ps_out, double *d_alpha, void *stream);
int pcs_genchain_lm_decide_bounded(pcs_genchain *h, const double *d_cost_old, const double *d_cost_new, const double *d_dvec, const double *d_gm, const double *d_delta,
                                   const double *d_ps, const uint8_t *d_fixed_eff, const double *d_alpha, int32_t *d_status, double *d_lambda, double *d_stats, void *stream);
int pcs_genchain_lm_trial(pcs_genchain *h, const pcs_lm_buffers *b, void *stream);
int pcs_genchain_set_option(pcs_genchain *h, const char *key, int64_t value);
/* The pieces of a trial as calls of their own — pcs_schur_prepare / pcs_schur_finish / pcs_lm_decide for the handle's layout — for a
 * loop the host steers (a sharded solve with a host-staged collective); pcs_schur_syrk, pcs_dense_spd_solve and pcs_schur_vtx take
 * sizes, not handles, and serve both kinds of handle. */
int pcs_genchain_schur_prepare(pcs_genchain *h, double *d_packed, const uint8_t *d_fixed, const double *d_lambda, double *d_linvt, double *d_u,
                               double *d_V, double *d_S, double *d_rhs, double *d_dvec, double *d_gm, int32_t *d_status, void *stream);
int pcs_genchain_schur_finish(pcs_genchain *h, const double *d_linvt, const double *d_u, const double *d_w, const double *d_xlead, const uint8_t *d_fixed,
                              double *d_delta, const double *d_ps_in, double *d_ps_out, void *stream);
int pcs_genchain_lm_decide(pcs_genchain *h, const double *d_cost_old, const double *d_cost_new, const double *d_dvec, const double *d_gm, const double *d_delta,
                           const double *d_ps, const uint8_t *d_fixed, int32_t *d_status, double *d_lambda, double *d_stats, void *stream);
int pcs_genchain_device_buffers(pcs_genchain *h, void **d_resid, void **d_jac);
int pcs_genchain_synchronize(pcs_genchain *h, void *stream);
int pcs_genchain_last_kernel_ms(pcs_genchain *h, float *slab_prep_ms, float *eval_ms);

/*
 * Legacy residual-only cost.
 * Replaces: bundle_adjustment_costfn / numpy_bundle_adjustment_costfn (compiled_helpers.py:518-549),
 * called once per candidate pose set during initialisation (template_handler.py:535-592).
 *   im_points  (n_imgs, n_keys, 3)  target points already transformed by each image's pose
 *   proj       (n_cams, 3, 4)       K [R|t] per camera
 *   intrinsics (n_cams, 3, 3), dists (n_cams, 5) = [k0, k1, p0, p1, k2]
 *   errors     (2N)                 [u0 err, v0 err, u1 err, ...] for the engine's detection table
 */
int pcs_legacy_cost(pcs_engine *h, const double *im_points, const double *proj, const double *intrinsics, const double *dists,
                    double *errors);

/* Block until everything queued on `stream` (NULL = engine stream) has finished. */
int pcs_synchronize(pcs_engine *h, void *stream);
/* Duration of the most recent evaluation's kernels, ms: each kernel's OWN start / stop events (hipExtLaunchKernelGGL on the
 * launch stream), so slab_prep_ms is the slab_prep kernel's duration without the gap to the next launch — the figure
 * rocprofv3 reports.  A one-launch step (option "fuse_prep") has no slab_prep kernel: slab_prep_ms = 0. */
int pcs_last_kernel_ms(pcs_engine *h, float *slab_prep_ms, float *eval_ms);
/* Mean kernel durations over the evaluations kept in the event ring (option "event_ring" = R keeps
 * the last R evaluations; the ring is reset when the option is set).  Used by bench.py for the
 * roofline figure: live HIP-event timing of every launch of the timed region. */
int pcs_kernel_ms_mean(pcs_engine *h, int64_t *count, float *slab_prep_ms, float *eval_ms);
/* The individual durations behind pcs_kernel_ms_mean, oldest first: up to `capacity` (slab_prep, eval) pairs are
 * written, *count = how many.  bench.py takes its median / min / mean from these (the reference's analogue is
 * the sample list of general_utils.benchmark(), utils/general_utils.py:62-104). */
int pcs_kernel_ms_samples(pcs_engine *h, int64_t capacity, float *slab_prep_ms, float *eval_ms, int64_t *count);
/* Tuning knobs ("variant", "wgs_per_cu", "tiles_per_wg", "event_ring", "timing_every", "compact_variant",
 * "fuse_prep" (-1 automatic / 0 / 1: one launch per step — every wave of the evaluation kernel prepares the R, t, dR/dr
 * slabs of its own tile instead of a slab_prep launch in front; automatic = tables in the reference's run order, FP64 outputs
 * at any size, float outputs up to "fuse_prep_max_n" detections; same slab element functions, same bits; the matrix-free
 * operators then need pcs_linearize), "lazy_done_event" (1: the engine's ordering event is recorded when somebody waits for
 * it, not after every step, for work on the engine's own or the default stream; 2: on caller streams too — the caller then keeps
 * the stream alive until it resets the option, which records what is pending; 0: after every enqueue), "timing_every" (0: no start / stop
 * events at all, neither around evaluations nor around normal-equations builds),
 * "matfree_lds" (how the transposed pcs_matfree operators — ops 1 to 4 — add up their n_params sums.  1, the default: in
 * workgroup-private LDS accumulators, flushed with one global f64 atomic per non-zero entry and workgroup — taken whenever they fit,
 * i.e. up to 13 740 parameters (150 KiB with the four reduction panels); larger strings take the other form on their own.  0: always
 * wave sums and global f64 atomics, no LDS (an A/B switch, and the way to test the form large strings get).  Same results up to the
 * order of the sums; op 0, J v, has no sums and ignores it),
 * "pack_indices" (1, the default: one packed 32-bit index word per detection where camera, image and key fit; 0: three int32 arrays;
 * takes effect at the next pcs_set_detections*),
 * "xcd_remap", "waves_per_wg", "normal_rows", "normal_imgkey_product",
 * "normal_imgkey_wgs_per_cu", "normal_sort_tables"; "normal_debug" is a bit mask of profiling switches of pcs_normal_equations — phases
 * or whole passes are skipped and the results are wrong while it is non-zero); see DESIGN.md.
 * Unknown keys -> PCS_ERR_ARG. */
int pcs_set_option(pcs_engine *h, const char *key, int64_t value);
/* Robust loss of the engine's normal equations, with the semantics of scipy.optimize.least_squares(loss=, f_scale=): applied to each
 * scalar residual f (the u and the v of a detection separately), z = (f / f_scale)^2, rho0 = f_scale^2 rho(z), rho1 = rho'(z),
 * rho2 = rho''(z) / f_scale^2, linearised as scipy's scale_for_robust_loss_function:  s = sqrt(max(rho1 + 2 rho2 f^2, EPS)),
 * row of J -> s J, f -> rho1 f / s.  A build then returns H = J~^T J~, g = J~^T r~ = J^T (rho1 f) and the cost word sum rho0
 * (= sum f^2 for the linear loss; the LM result's cost is half of it, scipy's OptimizeResult.cost).
 *   kind: PCS_LOSS_LINEAR (the default), PCS_LOSS_HUBER, PCS_LOSS_SOFT_L1, PCS_LOSS_CAUCHY, PCS_LOSS_ARCTAN.
 *   PCS_ERR_ARG for a NULL handle, an unknown kind, or an f_scale that is not finite and > 0 (the setting is then unchanged).
 * Affects every normal-equation build of the engine: pcs_normal_equations*, pcs_normal_blocks_device, pcs_lm_trial* and, through
 * those, the device-steered and sharded LM loops; both contraction orders (option "deterministic" keeps its same-bits guarantee).
 * Does NOT affect pcs_eval* and the compact paths (the drop-in closures keep returning the raw residuals and J), pcs_matfree (its
 * products use the raw J), nor generated chains (pcs_genchain_*).
 * The linear loss takes the builds' plain path: the same bits as an engine on which pcs_set_loss was never called. */
enum { PCS_LOSS_LINEAR = 0, PCS_LOSS_HUBER = 1, PCS_LOSS_SOFT_L1 = 2, PCS_LOSS_CAUCHY = 3, PCS_LOSS_ARCTAN = 4 };
int pcs_set_loss(pcs_engine *h, int kind, double f_scale);
/* The current setting (kind and f_scale may be NULL); PCS_ERR_ARG for a NULL handle. */
int pcs_get_loss(pcs_engine *h, int *kind, double *f_scale);
/* Noise weights of the engine's normal equations (since pcs_version() 112): inv_sigma[i] = 1 / sigma_i, the reciprocal pixel noise of detection i of the current
 * table, in table order (isotropic: one value for the u and the v of a detection).  A weight whitens in front of the loss of pcs_set_loss:
 * f -> f / sigma before rho, row of J -> (s / sigma) J, so a build minimises  sum rho(((f / sigma) / f_scale)^2) f_scale^2  — scipy's
 * least_squares(loss=, f_scale=) applied to the whitened residual f / sigma and Jacobian row J / sigma — and returns H = J~^T J~,
 * g = J~^T r~ and the cost word sum rho0, all of the whitened system (linear loss: sum (f / sigma)^2).
 *   inv_sigma = NULL clears the weights (n is then ignored).  Otherwise n must equal pcs_n_detections and every value must be finite
 *   and > 0: PCS_ERR_ARG if not, and for a NULL handle; a refused call leaves the previous weights in force.
 *   The weights belong to the detection table: pcs_set_detections* clears them.  The values are copied.
 * Affects what pcs_set_loss affects: pcs_normal_equations*, pcs_normal_blocks_device, pcs_lm_trial* and, through those, the
 * device-steered and sharded LM loops, in both contraction orders (option "deterministic" keeps its same-bits guarantee).
 * Does NOT affect pcs_eval* and the compact paths (the drop-in closures keep returning the raw residuals and J), pcs_matfree (its
 * products use the raw J), the group statistics (pcs_residual_stats*: raw pixels), nor generated chains (pcs_genchain_*).
 * Without weights the builds take the path the loss alone selects: the same bits as an engine on which pcs_set_weights was never called. */
int pcs_set_weights(pcs_engine *h, const double *inv_sigma, int64_t n);
/* The current weights: *n = their number (0 = none set); up to `capacity` of them are copied to inv_sigma.  inv_sigma or n may be NULL
 * (not both): pcs_get_weights(h, NULL, 0, &n) is the "are weights set" query.  PCS_ERR_ARG for a NULL handle or a negative capacity. */
int pcs_get_weights(pcs_engine *h, double *inv_sigma, int64_t capacity, int64_t *n);
/* Gaussian parameter prior of the engine's LM solve (since pcs_version() 114): what is known about a parameter, "about mean[i], give or
 * take sigma_i", over the parameter string p.  With w_i = inv_sigma[i] = 1 / sigma_i the objective becomes
 *     Phi(p) = sum over the detection rows of rho(...)  +  sum_i (w_i (p_i - mean[i]))^2 ,
 * the first sum being what the build computes (pcs_set_loss and pcs_set_weights included); the prior rows never pass through the loss
 * and are never whitened by the detections' sigma — scipy's extra rows (x - mu) / sigma, a Ceres prior block.  In a packed state
 * [A | B | C | g | cost] the diagonal entry of parameter i (A[i, i] of a leading column, the diagonal of its entity's C block for a
 * trailing one) gains w_i^2, g_i gains w_i^2 (p_i - mean[i]) and the cost word gains the sum; Marquardt scaling, the damped step, the
 * predicted reduction and gain ratio, gtol, ftol and the covariance all read those three places.
 *   pcs_set_prior   n must equal pcs_n_params; inv_sigma[i] finite and >= 0, 0 = no prior on that entry; mean[i] finite where
 *                   inv_sigma[i] > 0.  inv_sigma = NULL clears the prior.  PCS_ERR_ARG if not, and for a NULL handle; a refused call leaves
 *                   the previous prior in force.  The values are copied; only entries with inv_sigma > 0 cost device memory or time.
 *                   The prior belongs to the HANDLE: pcs_set_detections* keeps it.
 *   pcs_get_prior   *n = pcs_n_params when a prior is set, else 0; up to `capacity` values each go to mean and inv_sigma (any of the
 *                   three may be NULL, not all).
 *   pcs_prior_add_device   adds the prior at d_param_str to d_packed, a packed state of the handle's layout (pcs_normal_layout) built at
 *                   that string; asynchronous on `stream`.  No prior set: nothing is queued.
 * The RAW builds do NOT include the prior: pcs_normal_equations*, pcs_normal_blocks_device, pcs_eval* and pcs_matfree stay the sums over
 * the detections — they are what a loop over observation shards all-reduces, and the prior must enter ONCE, behind that sum.  It is
 * added by pcs_prior_add_device (the first state of a loop, after the all-reduce) and by pcs_lm_trial_finish, which — when a prior is
 * set — adds it to the trial state at the trial string in front of the decision, following flags[2] / PCS_LM_FIXED_TRIAL_BUFFER as the
 * decision does and behind the stop word like every kernel of a trial.  Every rank adds the same bits: no rank is special.  The stats
 * words [5] and [6] of a trial ("new / old sum r^2") are then the augmented sums.
 * The kernels (csrc/ba_prior.hpp) use plain adds — every destination has one writer — and sum the cost term in a fixed order in BOTH
 * contraction modes: option "deterministic" keeps its same-bits guarantee.  Up to 1 024 entries: one launch of one workgroup; more:
 * one launch of ceil(n / 1 024) workgroups and a one-workgroup launch that adds their partial sums in workgroup order.
 * Without a prior every entry point queues the launches it queued before and computes the same bits. */
int pcs_set_prior(pcs_engine *h, const double *mean, const double *inv_sigma, int64_t n);
int pcs_get_prior(pcs_engine *h, double *mean, double *inv_sigma, int64_t capacity, int64_t *n);
int pcs_prior_add_device(pcs_engine *h, const double *d_param_str, double *d_packed, void *stream);

/* Box bounds on the parameters of the engine's LM solve (since pcs_version() 118): lo[i] <= p[i] <= hi[i] over the parameter string,
 * -inf / +inf = none — what scipy least_squares(bounds=) is to the reference's call (optimisation_handling.py:88-98).  The method is an
 * active set plus a step cut at the first bound (csrc/ba_bounds.hpp); per trial, on the device, behind the stop word:
 *   1. from the CURRENT state: fixed_eff[i] = fixed[i] || lo[i] == hi[i] || (p[i] <= lo[i] && g[i] > 0) || (p[i] >= hi[i] && g[i] < 0)
 *      || (pinned[i] && p[i] on a bound); the Schur step reads fixed_eff where it reads `fixed` without bounds.
 *   2. behind the step d: alpha = min(1, min_i alpha_i), alpha_i the fraction of d[i] that takes p[i] to the bound it moves towards
 *      (ties: the lowest index); p_new = min(max(p + alpha d, lo), hi), the entry that sets alpha exactly on its bound; delta = p_new - p.
 *      An entry ON a bound whose step points out of the box (it would make alpha = 0) is PINNED instead: its component of the step is
 *      dropped, it takes no part in alpha, and — the handle's only memory — it joins the active set of the following trials until a
 *      trial is accepted.
 *   3. the decision: predicted reduction -(1 - alpha / 2) g'delta + 0.5 lambda delta'D delta; max |g| and |x| over fixed_eff (the
 *      projected gradient); a truncated trial (alpha < 1) triggers neither the ftol nor the xtol stop, counts towards the limits and
 *      takes the damping rule as usual, except that an accepted one never LOWERS lambda (the gain ratio of a cut step says nothing
 *      about the whole one).
 * With bounds set, pcs_lm_trial_build takes the NON-fused sequence plus two one-workgroup launches (the fused completion prepares the
 * slabs at the trial string in the launch that writes it); pcs_lm_trial_finish decides as in 3.  Without bounds every entry point
 * queues the launches it queued before and computes the same bits.
 *   pcs_set_bounds   n must equal pcs_n_params; no NaN, lo[i] <= hi[i] (lo[i] == hi[i] acts as fixed).  lo = hi = NULL clears the
 *                    bounds.  PCS_ERR_ARG if not, and for a NULL handle; a refused call leaves the previous bounds in force.  The values
 *                    are copied.  The bounds belong to the HANDLE: pcs_set_detections* keeps them.  Synchronises the device before it
 *                    overwrites lists a queued trial may still read; resets what pcs_bounds_trials reports.
 *   pcs_get_bounds   *n = pcs_n_params when bounds are set, else 0; up to `capacity` values each go to lo and hi (any of the three
 *                    outputs may be NULL).
 *   pcs_bounds_trials   after a loop of pcs_lm_trial* calls whose stream the caller has synchronised: alpha_active[2 k], [2 k + 1] =
 *                    alpha and the number of entries the bounds added to the mask in trial k + 1 (ctrl[8]), for the first n_trials
 *                    trials (NaN beyond the 4096 the handle records); *n_truncated = decided trials with alpha < 1 since pcs_set_bounds.
 *                    PCS_ERR_STATE without bounds.
 * For a loop the host steers (all pointers device memory; PCS_ERR_STATE without bounds):
 *   pcs_bounds_active_device    step 1 at the string d_ps and the packed state d_packed built there: d_fixed_eff (n_params bytes)
 *   pcs_bounds_truncate_device  step 2: d_delta in place, d_ps_out = the trial string (must differ from d_ps_in), *d_alpha
 *   pcs_bounds_active_sel_device / pcs_bounds_truncate_sel_device   the same two for a caller that keeps TWO states and a selector word
 *                               as pcs_lm_trial_build does: strings d_ps0 / d_ps1 and packed states d_packed0 / d_packed1; *d_sel != 0
 *                               names state 1 as the current one, the trial string is written into the other state's.
 *   pcs_lm_decide_bounded       pcs_lm_decide with step 3's predicted reduction; d_fixed_eff where pcs_lm_decide takes d_fixed.  The
 *                               ftol / xtol rule of a truncated trial is the caller's (it reads *d_alpha); an accepted trial clears the
 *                               handle's pins, and so does a void one. */
int pcs_set_bounds(pcs_engine *h, const double *lo, const double *hi, int64_t n);
int pcs_get_bounds(pcs_engine *h, double *lo, double *hi, int64_t capacity, int64_t *n);
int pcs_bounds_trials(pcs_engine *h, double *alpha_active, int64_t n_trials, int64_t *n_truncated);
int pcs_bounds_active_device(pcs_engine *h, const double *d_ps, const double *d_packed, const uint8_t *d_fixed, uint8_t *d_fixed_eff, void *stream);
int pcs_bounds_truncate_device(pcs_engine *h, const double *d_ps_in, double *d_delta, double *d_ps_out, double *d_alpha, void *stream);
int pcs_bounds_active_sel_device(pcs_engine *h, const double *d_ps0, const double *d_ps1, const double *d_packed0, const double *d_packed1, const uint8_t *d_fixed,
                                 uint8_t *d_fixed_eff, const int32_t *d_sel, void *stream);
int pcs_bounds_truncate_sel_device(pcs_engine *h, double *d_ps0, double *d_ps1, double *d_delta, double *d_alpha, const int32_t *d_sel, void *stream);
int pcs_lm_decide_bounded(pcs_engine *h, const double *d_cost_old, const double *d_cost_new, const double *d_dvec, const double *d_gm, const double *d_delta,
                          const double *d_ps, const uint8_t *d_fixed_eff, const double *d_alpha, int32_t *d_status, double *d_lambda, double *d_stats, void *stream);
/*
 * Batched n-view triangulation.
 * Replaces: nb_triangulate_full (compiled_helpers.py:609-643) = per point nb_undistort (ch:409-431) +
 *           nb_triangulate_nviews (ch:645-663, smallest right singular vector of the 3n x (4+n) DLT
 *           matrix); front end CameraSet.multi_cam_triangulate (cameras/camera_set.py:343-402), which calls it once
 *           per set of frames with the same cameras.
 * A pcs_triangulator owns the camera table, device copies of the observations, the kernel's scratch and (optionally)
 * the output, so repeated calls allocate nothing:
 *   pcs_tri_set_cameras              proj (n_cams,3,4), intrinsics (n_cams,3,3), dists (n_cams,5) = [k0,k1,p0,p1,k2]
 *   pcs_tri_set_observations         host arrays, copied: cam (n_obs) int32, uv (n_obs,2) sorted by point; point j owns
 *                                    rows [start_inds[j], start_inds[j+1]) (n_pts+1 entries, like the reference's);
 *                                    cameras are range-checked -> PCS_ERR_RANGE
 *   pcs_tri_set_observations_device  the same arrays already in device memory (caller-owned, not copied, not checked)
 *   pcs_tri_run                      queue the kernel on `stream` (NULL = the handle's own stream); d_pts = device
 *                                    buffer (n_pts,3) of the caller, or NULL = handle-owned output
 *   pcs_tri_points                   copy the handle-owned output to the host (blocking; PCS_ERR_STATE when the last run
 *                                    wrote to a caller buffer instead)
 * Fewer than two views: start_inds may repeat a value (a point without views, also at the end of the table, where its start equals
 * n_obs) or advance by one.  Such a point is not determined; pcs_tri_run writes three NaNs for it, whichever kernel runs, reads no
 * observation outside [0, n_obs) for it, and the points around it keep the bits they have without it.  pcs_tri_refine leaves it at
 * PCS_TRI_REFINE_NOT_REFINED with NaN points, NaN RMS values and its view count.
 * Runs on different streams are ordered by the handle (scratch and output are shared): an event recorded after every run
 * is waited for by the next run, by pcs_tri_points and by the setters, whatever stream the run was queued on.
 * pcs_triangulate is the stateless convenience form (temporary handle: allocations and copies on every call).
 */
typedef struct pcs_triangulator pcs_triangulator;
int pcs_tri_create(pcs_triangulator **out, int device, int64_t n_cams);
int pcs_tri_destroy(pcs_triangulator *t);
int pcs_tri_set_cameras(pcs_triangulator *t, const double *proj, const double *intrinsics, const double *dists);
int pcs_tri_set_observations(pcs_triangulator *t, int64_t n_obs, const int32_t *cam, const double *uv, int64_t n_pts, const int64_t *start_inds);
int pcs_tri_set_observations_device(pcs_triangulator *t, int64_t n_obs, const int32_t *d_cam, const double *d_uv, int64_t n_pts,
                                    const int64_t *d_start_inds);
/* The grouping CameraSet.multi_cam_triangulate does in front of nb_triangulate_full (cameras/camera_set.py:371-378: two np.unique calls over
 * the (image, key...) columns — which features are seen by more than one camera, their rows in table order, start indices in order of
 * first appearance), on the device: n table rows as caller-owned device arrays (camera index, dense feature id in [0, n_features),
 * measurement), grouped by feature like TargetDetection.get_data returns them -> the handle's current observations (pcs_tri_run next).
 * *n_pts / *n_kept: features kept / their rows.  *grouped = 0 (nothing set): a feature's rows are not consecutive — group on the host
 * (the reference's consecutive slices then mix features; the host mirror reproduces that).  One host synchronisation. */
int pcs_tri_group_device(pcs_triangulator *t, int64_t n, const int32_t *d_cam, const int32_t *d_feat, const double *d_uv, int64_t n_features,
                         int64_t *n_pts, int64_t *n_kept, int32_t *grouped, void *stream);
int pcs_tri_run(pcs_triangulator *t, double *d_pts, void *stream);
/* What pcs_tri_run launches for this handle (read-only; since pcs_version() 109): out[0] lanes per point (1, 2, 4, 8 or 16), out[1]
 * views per lane kept in registers (0 for the kernel that keeps every view in the global scratch), out[2] 1 for the register kernel and
 * 0 for the scratch kernel, out[3] 1 when the points are visited in order of their view count and 0 for table order.  The geometry is
 * fixed at pcs_tri_create from the environment switches PCS_TRI_LANES (1, 2, 4, 8, 16; anything else: 4), PCS_TRI_VARIANT (0: scratch
 * kernel; 3: eight register views at four lanes; anything else: the default) and PCS_TRI_NO_SORT (set: table order); the default is
 * {4, 6, 1, 1}.  The switches exist for A/B timing and tests: every geometry computes the same points to rounding. */
int pcs_tri_launch_config(pcs_triangulator *t, int32_t out[4]);
int pcs_tri_points(pcs_triangulator *t, double *pts);
int pcs_tri_synchronize(pcs_triangulator *t, void *stream);
int pcs_tri_last_kernel_ms(pcs_triangulator *t, float *kernel_ms);
int pcs_triangulate(int device, int64_t n_obs, const int32_t *cam, const double *uv, int64_t n_pts, const int64_t *start_inds,
                    int64_t n_cams, const double *proj, const double *intrinsics, const double *dists, double *pts,
                    float *kernel_ms);
/* Reprojection-error refinement of the triangulation (csrc/ba_tri_refine.hpp).  Since pcs_version() 104.
 * For point j with views v = (camera c_v, measurement uv_v): minimise sum_v || uv_v - pi_{c_v}(X) ||^2 over X, pi_c = the reference's
 * Camera.project_points(distort=True) (cameras/camera.py:242-272): h = P_c [X; 1], pixel (h0 / h2, h1 / h2), then the Brown-Conrady
 * distortion nb_distort_prealloc (camera.py:32-56) with fx = K00, fy = K11, (cx, cy) = K[0:2, 2] and the table's [k0, k1, p0, p1, k2].
 * Per point Levenberg-Marquardt on the 3 x 3 system (H + lam diag(H)) d = g, H = J'J, g = J'r, starting from the DLT point of the last
 * pcs_tri_run on the same cameras and observations (read on the device where that run wrote it: the handle's output or the caller's
 * d_pts, which must still hold it).  A trial is accepted when its cost is lower and every view has depth h2 > 0, so a returned point
 * never costs more than its start.  Stops: max_iter trials, relative cost decrease <= ftol, step <= xtol (xtol + |X|), max |g| <= gtol.
 *   pcs_tri_refine   queue the refinement on `stream` (NULL = the handle's stream), ordered after the run like the runs among themselves.
 *                    Outputs (device buffers of the caller, or NULL = handle-owned): d_pts (n_pts, 3) refined points; d_rms (n_pts, 2)
 *                    RMS reprojection error sqrt(sum_v |r_v|^2 / n_v) at the returned point and at the DLT point; d_info (n_pts, 3)
 *                    int32 {trials used, status PCS_TRI_REFINE_*, views}; with flags PCS_TRI_REFINE_RESIDUALS, d_resid (n_obs, 2)
 *                    residuals uv - pi(X) at the returned points in the handle's observation order.  PCS_ERR_ARG: NULL handle,
 *                    max_iter < 0, a negative or non-finite tolerance, unknown flags; PCS_ERR_STATE: no run since the cameras or
 *                    observations were last set.
 *   pcs_tri_refined  copy the handle-owned outputs of the last refinement to the host (any pointer may be NULL; blocking).
 *                    PCS_ERR_STATE when there was no refinement since the last run or a requested output went to a caller buffer.
 *   pcs_tri_last_refine_ms  device time of the last refinement kernel.
 * Defaults of the Python front end (pycamset_amd.compiled_helpers.REFINE_DEFAULTS): max_iter 10, ftol 1e-10, xtol 1e-10, gtol 0. */
#define PCS_TRI_REFINE_RESIDUALS 1
enum {
    PCS_TRI_REFINE_NOT_REFINED = 0,   /* non-finite DLT start (a point with fewer than two views included) or a start behind a camera: the DLT point is returned unchanged */
    PCS_TRI_REFINE_CONVERGED = 1,     /* ftol, xtol or gtol */
    PCS_TRI_REFINE_MAX_ITER = 2,      /* max_iter trials used */
    PCS_TRI_REFINE_NO_DECREASE = 3    /* the damping grew past 1e10 without a lower cost, or the damped system lost definiteness */
};
enum { PCS_TRI_OUT_POINTS = 1, PCS_TRI_OUT_RMS = 2, PCS_TRI_OUT_INFO = 4, PCS_TRI_OUT_RESIDUALS = 8 };
int pcs_tri_refine(pcs_triangulator *t, int max_iter, double ftol, double xtol, double gtol, int flags, double *d_pts, double *d_rms,
                   int32_t *d_info, double *d_resid, void *stream);
int pcs_tri_refined(pcs_triangulator *t, double *pts, double *rms, int32_t *info, double *resid);
int pcs_tri_last_refine_ms(pcs_triangulator *t, float *kernel_ms);
/* Robust loss of the refinement (since pcs_version() 113).  The kinds, the formulas and the validation are those of pcs_set_loss, applied
 * to each scalar residual (u and v separately): H = sum s^2 J'J, g = sum J' rho1 f.  The cost the accept rule, ftol and the test of the
 * start look at is sum rho0; the depth test, the damping, xtol, gtol (on the robust g) and the statuses keep their rules.  d_rms stays the
 * plain pixel RMS and d_resid the raw residuals.  The setting belongs to the handle and survives new cameras and observations;
 * PCS_LOSS_LINEAR, the default, launches the kernel of a handle on which no loss was ever set.
 *   pcs_tri_set_refine_loss  mirrors pcs_set_loss.  PCS_ERR_ARG (the previous setting stays in force): NULL handle, a kind outside
 *                            PCS_LOSS_*, an f_scale that is not finite and > 0.
 *   pcs_tri_get_refine_loss  mirrors pcs_get_loss (either pointer may be NULL).
 *   pcs_tri_refine_costs     mirrors pcs_tri_refined for one more output: cost (n_pts, 2) = 0.5 sum rho0 (scipy's cost) at the returned
 *                            point and at the DLT point, always handle-owned (blocking).  A point that was not refined has the cost
 *                            of its unchanged start in both columns, as its RMS has: finite for a start behind a camera, NaN for a
 *                            non-finite start and for a point without views — under every loss, linear included.  After a LINEAR
 *                            refinement the costs are derived in this call, 0.5 n rms^2 from the RMS that refinement wrote (read on
 *                            the device where it wrote it: the handle's output or the caller's d_rms, which must still hold it);
 *                            the refinement itself queues what it queued before a loss existed.  PCS_ERR_ARG: NULL handle or array;
 *                            PCS_ERR_STATE: no refinement since the last run. */
int pcs_tri_set_refine_loss(pcs_triangulator *t, int kind, double f_scale);
int pcs_tri_get_refine_loss(pcs_triangulator *t, int *kind, double *f_scale);
int pcs_tri_refine_costs(pcs_triangulator *t, double *cost);
/* View-pair consensus in front of the triangulation (csrc/ba_tri_consensus.hpp; since pcs_version() 116), opt-in: what the two-view RANSAC
 * of COLMAP's and OpenCV's n-view triangulation is to their DLT.  One mismatched view drags the DLT start of its point, and the refinement
 * starts there.  With the stage on, n_hypotheses PAIRS of views per point are triangulated by the same kernel pcs_tri_run launches
 * (pcs_tri_launch_config), each candidate is scored on every view of the point by sum min(e^2, inlier_px^2) — e the reprojection error in
 * the measured pixels, the projection of pcs_tri_refine; inlier_px^2 for a view with a non-finite measurement or projection or a depth
 * <= 0 — and the DLT of pcs_tri_run and pcs_tri_refine then work on the views within inlier_px of the best candidate (ties: the lower
 * hypothesis).  A point with V views takes all V (V - 1) / 2 pairs in lexicographic order when they are at most n_hypotheses; otherwise
 * the pairs come from a counter-based sampler keyed by (seed, index of the point in the handle's observations, V, hypothesis): one
 * 64-bit draw r gives a = r mod V and b = (r >> 32) mod (V - 1), bumped past a.  The hypothesis count is fixed, so two runs agree bit for
 * bit, and a table without outliers gives the bits of the plain run.  The stage waits for nothing on the host.
 *   pcs_tri_set_consensus     n_hypotheses = 0 (the default) turns the stage off: pcs_tri_run and pcs_tri_refine then queue what they
 *                             always queued and allocate nothing more.  PCS_ERR_ARG: NULL handle, a negative count, n_hypotheses > 256,
 *                             inlier_px not finite or <= 0; a refused call keeps the previous setting.  The setting belongs to the
 *                             handle and survives new cameras and observations, however they are set (host, device,
 *                             pcs_tri_group_device).
 *   pcs_tri_get_consensus     the setting in force (any pointer may be NULL)
 *   pcs_tri_consensus_results copy what the stage of the last run found to the host (blocking, any pointer may be NULL): inlier (n_obs)
 *                             one flag per observation; cinfo (n_pts, 4) int32 {inliers, winning hypothesis or -1, hypotheses with a
 *                             finite candidate, consensus used}; score (n_pts) the winner's sum (+inf: no finite candidate, NaN:
 *                             consensus not used).  A point with fewer than 3 views takes the plain path (all flagged, consensus used
 *                             = 0); a point without a finite candidate, or whose winner has fewer than 2 inliers, keeps no row (inliers
 *                             0) and is not determined: three NaNs, like a point without views; a NaN measurement is never an inlier.
 *                             With the stage on, d_rms of pcs_tri_refine is over the inliers, d_info keeps the point's full view count,
 *                             d_resid holds the residuals of ALL observations at the returned point, and pcs_tri_refine_costs counts
 *                             the inliers.  pcs_tri_last_kernel_ms and pcs_tri_last_refine_ms include the stage's kernels.
 *                             PCS_ERR_STATE when the last run had no consensus stage. */
int pcs_tri_set_consensus(pcs_triangulator *t, int n_hypotheses, double inlier_px, uint64_t seed);
int pcs_tri_get_consensus(pcs_triangulator *t, int *n_hypotheses, double *inlier_px, uint64_t *seed);
int pcs_tri_consensus_results(pcs_triangulator *t, uint8_t *inlier, int32_t *cinfo, double *score);

/* ------------------------------------------------------------------------------------------------
 * Batched target-pose estimation, PnP (csrc/ba_pnp.hpp).  Since pcs_version() 105.
 * Replaces: AbstractTarget.target_pose_in_cam_image (calibration_targets/abstract_target.py:345-405: at least 6 points,
 *           cv2.solvePnPGeneric, the solution of lowest error), called per camera and image by estimate_camera_relative_poses
 *           (optimisation/template_handler.py:484-491) in front of calc_initial_params (template_handler.py:302-346).
 * A view is the set of detections of one (camera, image) pair.  Per view: the measurements are undistorted (five fixed-point steps) for
 * a linear start that needs no prior (planar views, lambda_min / lambda_mid of the template points' scatter < 1e-3: homography;
 * others: 3 x 4 DLT), then a 6-parameter Levenberg-Marquardt minimises sum || uv - pi(R X + t) ||^2 in the measured pixels with the full
 * Brown-Conrady model; planar views are also refined from the second pose of the planar ambiguity and the lower cost is kept (the
 * reference's argmin over solvePnPGeneric's solutions).  Pose convention: X_cam = R(r) X_target + t, r a Rodrigues vector, |r| <= pi.
 * Damping, accept rule and stops are those of pcs_tri_refine (the step is compared with the Frobenius size of [R | t]).
 *   pcs_pnp_create            n_cams cameras, a template of n_keys points
 *   pcs_pnp_set_cameras       intr (n_cams, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2], the engine's intrinsics slab
 *                             (template_handler.py:321-329 builds the same rows from the camera set)
 *   pcs_pnp_set_template      points (n_keys, 3): target.point_data flattened (template_handler.py:511)
 *   pcs_pnp_set_observations  host arrays, copied: key (n_obs) int32, uv (n_obs, 2), sorted by view; view j owns rows
 *                             [start_inds[j], start_inds[j+1]) and belongs to camera view_cam[j]; keys and cameras are range-checked
 *                             -> PCS_ERR_RANGE (abstract_target.py:360-375 gathers the same per image)
 *   pcs_pnp_run               queue the kernels on `stream` (NULL = the handle's stream).  A view with fewer than min_points
 *                             observations (the reference: 6, abstract_target.py:377), a non-finite start or a start behind the camera
 *                             is not estimated: NaN pose, status 0.  Outputs (device buffers of the caller, or NULL = handle-owned):
 *                             d_pose (n_views, 6); d_pose_init (n_views, 6) the linear start; d_pose_alt (n_views, 6) the second planar
 *                             start (NaN for 3-D views); d_rms (n_views, 2) RMS reprojection error at the returned pose and at the
 *                             start, pixels; d_info (n_views, 3) int32 {trials used, status PCS_PNP_*, observations}; with flags
 *                             PCS_PNP_RESIDUALS, d_resid (n_obs, 2) residuals at the returned pose in observation order.
 *                             PCS_ERR_ARG: NULL handle, max_iter < 0, a negative or non-finite tolerance, min_points < 1, unknown flags.
 *   pcs_pnp_results           copy handle-owned outputs of the last run to the host (any pointer may be NULL; blocking)
 *                             (replaces the Mat_ac array of template_handler.py:485-491)
 *   pcs_pnp_last_kernel_ms    device time of the last run: ordering of the views, start and LM kernels, and the consensus stage
 *                             when it is on.  PCS_ERR_STATE when the last run had no views and so queued nothing.
 *
 * Consensus sampling (csrc/ba_pnp_consensus.hpp; since pcs_version() 115), opt-in: what cv2.solvePnPRansac is to cv2.solvePnPGeneric,
 * at the same place in the pipeline (abstract_target.py:345-405).  One detection with a wrong id bends the linear start of its view;
 * with the stage on, n_hypotheses samples of sample_size detections per view are fitted by the same linear start, both of its poses are
 * scored on every detection of the view by sum min(e^2, inlier_px^2), and start and LM then run on the detections within inlier_px of
 * the best candidate.  The sampler is counter-based, keyed by (seed, camera, observations of the view, hypothesis); the hypothesis
 * count is fixed, so two runs agree bit for bit, and a table without outliers gives the bits of the plain run.
 *   pcs_pnp_set_consensus     n_hypotheses = 0 (the default) turns the stage off: pcs_pnp_run then queues what it always queued and
 *                             allocates nothing more (cv2.solvePnPGeneric).  Otherwise cv2.solvePnPRansac's iterationsCount,
 *                             its minimal sample (here 4 <= sample_size <= 16: the linear start, no P3P), reprojectionError and the
 *                             seed of its generator.  PCS_ERR_ARG: NULL handle, a negative count, n_hypotheses > 4096, sample_size
 *                             outside [4, 16], inlier_px not finite or <= 0; a refused call keeps the previous setting.
 *   pcs_pnp_get_consensus     the setting in force (any pointer may be NULL; cv2.solvePnPRansac's arguments, which it does not keep)
 *   pcs_pnp_consensus_results copy what the stage of the last run found to the host (cv2.solvePnPRansac's `inliers`; blocking, any
 *                             pointer may be NULL): inlier (n_obs) one flag per observation; cinfo (n_views, 4) int32 {inliers, winning
 *                             hypothesis or -1, hypotheses with a finite candidate, consensus used}; score (n_views) the winner's
 *                             sum min(e^2, inlier_px^2) (+inf: no finite candidate, NaN: consensus not used).  A view with fewer
 *                             observations than sample_size takes the plain path (all flagged, consensus used = 0); a view whose
 *                             best candidate has fewer than min_points inliers, or no finite candidate, is not estimated; a NaN
 *                             measurement is never an inlier.  With the stage on, d_rms is over the inliers, d_info keeps the
 *                             view's observation count, d_resid holds the residuals of ALL observations at the returned pose.
 *                             PCS_ERR_STATE when the last run had no consensus stage.
 */
typedef struct pcs_pose_estimator pcs_pose_estimator;
#define PCS_PNP_RESIDUALS 1
enum {
    PCS_PNP_NOT_ESTIMATED = 0,   /* too few observations, a non-finite start or a start behind the camera: the pose is NaN */
    PCS_PNP_CONVERGED = 1,       /* ftol, xtol or gtol */
    PCS_PNP_MAX_ITER = 2,        /* max_iter trials used */
    PCS_PNP_NO_DECREASE = 3      /* the damping grew past 1e10 without a lower cost, or the damped system lost definiteness */
};
enum { PCS_PNP_OUT_POSE = 1, PCS_PNP_OUT_POSE_INIT = 2, PCS_PNP_OUT_POSE_ALT = 4, PCS_PNP_OUT_RMS = 8, PCS_PNP_OUT_INFO = 16, PCS_PNP_OUT_RESIDUALS = 32 };
int pcs_pnp_create(pcs_pose_estimator **out, int device, int64_t n_cams, int64_t n_keys);
int pcs_pnp_destroy(pcs_pose_estimator *p);
int pcs_pnp_set_cameras(pcs_pose_estimator *p, const double *intr);
int pcs_pnp_set_template(pcs_pose_estimator *p, const double *points);
int pcs_pnp_set_observations(pcs_pose_estimator *p, int64_t n_obs, const int32_t *key, const double *uv, int64_t n_views, const int64_t *start_inds,
                             const int32_t *view_cam);
int pcs_pnp_run(pcs_pose_estimator *p, int max_iter, double ftol, double xtol, double gtol, int min_points, int flags, double *d_pose,
                double *d_pose_init, double *d_pose_alt, double *d_rms, int32_t *d_info, double *d_resid, void *stream);
int pcs_pnp_results(pcs_pose_estimator *p, double *pose, double *pose_init, double *pose_alt, double *rms, int32_t *info, double *resid);
int pcs_pnp_last_kernel_ms(pcs_pose_estimator *p, float *kernel_ms);
int pcs_pnp_set_consensus(pcs_pose_estimator *p, int n_hypotheses, int sample_size, double inlier_px, uint64_t seed);
int pcs_pnp_get_consensus(pcs_pose_estimator *p, int *n_hypotheses, int *sample_size, double *inlier_px, uint64_t *seed);
int pcs_pnp_consensus_results(pcs_pose_estimator *p, uint8_t *inlier, int32_t *cinfo, double *score);

/* ------------------------------------------------------------------------------------------------
 * Two-view relative pose by consensus (csrc/ba_twoview.hpp).  Since pcs_version() 119.
 * The host counterpart is cv2.findEssentialMat(..., RANSAC) followed by cv2.recoverPose: the one estimate of target-free bundle
 * adjustment (FreePointBundleHandler) that needs no 3-D knowledge.  The reference has none (free_point_handler.py:235 asks the
 * primitive for a pose_end it lacks).
 * A pair p of cameras (a, b), a < b, owns rows [start_inds[p], start_inds[p+1]) of a correspondence table (uv_a, uv_b) in measured
 * pixels.  Per pair: both pixels are undistorted (five fixed-point steps); n_hypotheses samples of eight rows are fitted by the
 * normalised eight-point method and projected onto the essential manifold; every hypothesis is scored on all rows of the pair by
 * sum min(e^2, inlier_px^2), e^2 the Sampson distance in undistorted pixels; the lowest score wins (ties: the lower hypothesis); the
 * same fit over the winner's inliers gives E, and of its four (R, +-t) the one with the most inliers in front of both cameras is
 * returned (ties: the lower candidate).  The sampler is counter-based, keyed by (seed, pair index, rows of the pair, hypothesis);
 * the hypothesis count is fixed and every sum has a fixed order: two runs agree bit for bit, and a pair's result does not depend
 * on the other pairs of the table.  The eight-point method degenerates for coplanar points and for a pure rotation: status,
 * n_front and parallax report that.
 *   pcs_twoview_create             n_cams >= 2 cameras
 *   pcs_twoview_set_cameras        intr (n_cams, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2]
 *   pcs_twoview_set_correspondences  host arrays, copied: uv_a, uv_b (n_corr, 2), start_inds (n_pairs + 1), pair_cams (n_pairs, 2)
 *                                  int32.  Checked without touching the device, and a refused call keeps the previous table:
 *                                  PCS_ERR_RANGE a camera outside [0, n_cams); PCS_ERR_ARG a >= b, start_inds not running from 0 to
 *                                  n_corr or decreasing, a non-finite pixel.
 *   pcs_twoview_set_consensus      1 <= n_hypotheses <= 256 (else PCS_ERR_RANGE; default 64), inlier_px finite and > 0 (else
 *                                  PCS_ERR_ARG; default 2), seed.  A refused call keeps the previous setting.
 *   pcs_twoview_get_consensus      the setting in force (any pointer may be NULL)
 *   pcs_twoview_set_solver         since pcs_version() 120, opt-in (csrc/ba_fivepoint.hpp).  solver: PCS_TWOVIEW_EIGHT_POINT (default,
 *                                  everything above) or PCS_TWOVIEW_FIVE_POINT, else PCS_ERR_ARG; refine_iters in [0, 50] (default
 *                                  0), else PCS_ERR_RANGE.  A refused call keeps the previous setting.
 *                                  FIVE_POINT: for scenes that are (mostly) one plane, where the eight-point method degenerates.
 *                                  Every hypothesis is Nister's five-point solver on five sampled rows, in normalised camera
 *                                  coordinates: up to ten essential matrices, the real roots of a degree-10 polynomial found by a
 *                                  Sturm chain with fixed iteration counts.  A candidate's score is the smallest, over its four
 *                                  (R, +-t), of sum min(e^2, inlier_px^2) in which a row that is not in front of both cameras counts
 *                                  inlier_px^2 (ties: the lower candidate); the lowest score of a pair wins (ties: the lower
 *                                  hypothesis, then the lower root).  Inlier flags: e^2 <= inlier_px^2 and in front under the
 *                                  winner.  There is no refit over the inliers (it degenerates on a plane): the winner's (R, t) is
 *                                  the model.  Statuses: TOO_FEW below max(5, min_points) rows; DEGENERATE without a usable
 *                                  candidate or with fewer than 6 inliers; info's winning hypothesis stays the sample's index.
 *                                  refine_iters > 0, with either solver: behind the final model at most refine_iters trials of a
 *                                  5-parameter Levenberg-Marquardt on R <- exp(omega) R, t <- exp(nu) t (nu across t) over the
 *                                  signed Sampson residuals of the inliers, with the damping, accept and stop rules of
 *                                  pcs_tri_refine (ftol = xtol = 1e-10).  The inlier flags stay the winner's; the count in front, the
 *                                  RMS and the parallax are taken at the refined pose.  Its time counts under "final".
 *   pcs_twoview_get_solver         the setting in force (any pointer may be NULL)
 *   pcs_twoview_run                queue the kernels on `stream` (NULL = the handle's stream).  group_lanes: 16 or 64 lanes per
 *                                  pair in the scoring, selection and final kernels, 0 = 64 from a mean of 256 rows per pair on.
 *                                  flags: none defined, pass 0.  d_T (n_pairs, 12), a device buffer of the caller or NULL =
 *                                  handle-owned: [R | t] row-major, X_b = R X_a + t, |t| = 1; NaN unless the status is OK.
 *   pcs_twoview_results            copy the outputs of the last run to the host (any pointer may be NULL; blocking): T (n_pairs, 12);
 *                                  info (n_pairs, 5) int32 {rows, inliers, inliers in front of both cameras, status
 *                                  PCS_TWOVIEW_*, winning hypothesis or -1}; stats (n_pairs, 3) {the winner's score (+inf: no
 *                                  usable hypothesis, NaN: too few rows), RMS Sampson distance over the inliers at the final E,
 *                                  parallax: RMS angle between the two rays of the front inliers, radians} (the last two NaN unless
 *                                  OK); inlier (n_corr) one flag per row, e^2 <= inlier_px^2 at the winning hypothesis.
 *   pcs_twoview_last_kernel_ms     device time of the stages of the last run, kernel_ms[5] = {undistort, hypotheses, scores,
 *                                  selection, final}.  PCS_ERR_STATE when the last run had no pairs and so queued nothing.
 */
typedef struct pcs_two_view pcs_two_view;
enum {
    PCS_TWOVIEW_OK = 0,
    PCS_TWOVIEW_TOO_FEW = 1,        /* fewer than max(8, min_points) rows (five-point solver: max(5, min_points)) */
    PCS_TWOVIEW_DEGENERATE = 2,     /* no usable hypothesis, fewer than 8 inliers (five-point solver: 6), or the fit over the inliers lost rank */
    PCS_TWOVIEW_NO_CHEIRALITY = 3   /* no inlier in front of both cameras */
};
enum { PCS_TWOVIEW_EIGHT_POINT = 0, PCS_TWOVIEW_FIVE_POINT = 1 };
enum { PCS_TWOVIEW_OUT_T = 1, PCS_TWOVIEW_OUT_INFO = 2, PCS_TWOVIEW_OUT_STATS = 4, PCS_TWOVIEW_OUT_INLIER = 8 };
int pcs_twoview_create(pcs_two_view **out, int device, int64_t n_cams);
int pcs_twoview_destroy(pcs_two_view *p);
int pcs_twoview_set_cameras(pcs_two_view *p, const double *intr);
int pcs_twoview_set_correspondences(pcs_two_view *p, int64_t n_corr, const double *uv_a, const double *uv_b, int64_t n_pairs, const int64_t *start_inds,
                                    const int32_t *pair_cams);
int pcs_twoview_set_consensus(pcs_two_view *p, int n_hypotheses, double inlier_px, uint64_t seed);
int pcs_twoview_get_consensus(pcs_two_view *p, int *n_hypotheses, double *inlier_px, uint64_t *seed);
int pcs_twoview_set_solver(pcs_two_view *p, int solver, int refine_iters);
int pcs_twoview_get_solver(pcs_two_view *p, int *solver, int *refine_iters);
int pcs_twoview_run(pcs_two_view *p, int min_points, int group_lanes, int flags, double *d_T, void *stream);
int pcs_twoview_results(pcs_two_view *p, double *T, int32_t *info, double *stats, uint8_t *inlier);
int pcs_twoview_last_kernel_ms(pcs_two_view *p, float *kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Rigid / similarity registration of 3-D point sets, absolute orientation (csrc/ba_align.hpp).  Since pcs_version() 121.
 * Replaces: n_estimate_rigid_transform (optimisation/compiled_helpers.py:727-762), a Kabsch fit of one pair of point sets by an SVD, and
 *           what its caller SelfBundleHandler.apply_gauge_transform (optimisation/self_bundle_handler.py:339-410) needs from it; batched,
 *           weighted, with the Umeyama scale and an opt-in consensus stage, which the reference lacks.
 * Problem j owns rows [start_inds[j], start_inds[j+1]) of a table of source points x, destination points y and optional weights w.  Per
 * problem: (s, R, t) with y ~ s R x + t in the weighted least-squares sense, s = 1 for the rigid model.  A row with a non-finite
 * coordinate or with w = 0 takes no part and is not counted.  Centroids first, then the cross-covariance S of the centred rows; the
 * rotation is Horn's unit quaternion, the largest eigenvector of the symmetric 4 x 4 N(S) by cyclic Jacobi, a proper rotation for planar
 * and for mirrored sets alike; s = l1 / sum w |x~|^2; t = y_mean - s R x_mean.  conditioning = (l1 - l2) / (l1 - l4) of N's eigenvalues
 * = (sigma_2 +- sigma_3) / (sigma_1 + sigma_2) of S's singular values: 0 for collinear points.  No floating-point atomics, every sum in
 * a fixed order: for a given group width two runs give the same bits, and a problem's result does not depend on its neighbours.
 *   pcs_align_create            a handle on `device` (no counterpart)
 *   pcs_align_destroy           frees the handle (no counterpart)
 *   pcs_align_set_points        host arrays, copied: src, dst (n_rows, 3), weights (n_rows) or NULL = 1 (compiled_helpers.py:727-762 takes
 *                               v0, v1 of one problem, unweighted), start_inds (n_problems + 1).  Checked without touching the device, and
 *                               a refused call keeps the previous table: PCS_ERR_ARG start_inds not running from 0 to n_rows or
 *                               decreasing, a weight that is negative or not finite.  Non-finite coordinates are data: the row is skipped.
 *   pcs_align_set_consensus     opt-in, in front of the fit (no counterpart).  0 <= n_hypotheses <= 256 (else PCS_ERR_RANGE; default 0 =
 *                               off), inlier_dist finite and > 0 when n_hypotheses > 0 (else PCS_ERR_ARG), seed.  Every hypothesis is the
 *                               same closed form on three rows drawn by the counter-based sampler of pcs_pnp_set_consensus, keyed by
 *                               (seed, problem index, rows of the problem, hypothesis); it is scored on all rows of the problem by
 *                               sum min(d^2, inlier_dist^2), d = |y - s R x - t|, a skipped row counting inlier_dist^2; the lowest
 *                               score wins (ties: the lower hypothesis); the fit then runs on the rows with d <= inlier_dist at the
 *                               winner.  A problem of fewer than three rows skips the stage.  A refused call keeps the previous setting.
 *   pcs_align_get_consensus     the setting in force (any pointer may be NULL)
 *   pcs_align_run               queue the kernels on `stream` (NULL = the handle's stream); the fit of compiled_helpers.py:727-762 for every
 *                               problem.  model: PCS_ALIGN_RIGID or PCS_ALIGN_SIMILARITY; min_points >= 3; rank_tol in [0, 1): a problem
 *                               whose conditioning is <= rank_tol is DEGENERATE; group_lanes: 16 or 64 lanes per problem, 0 = 64 from a
 *                               mean of 256 rows per problem on; flags: none defined, pass 0.  d_T (n_problems, 12), a device buffer of
 *                               the caller or NULL = handle-owned: [R | t] row-major; NaN unless the status is OK.
 *   pcs_align_results           copy the outputs of the last run to the host (any pointer may be NULL; blocking; no counterpart): T
 *                               (n_problems, 12); scale (n_problems); info (n_problems, 4) int32 {rows used, inliers (rows used without
 *                               consensus), status PCS_ALIGN_*, winning hypothesis or -1}; stats (n_problems, 3) {weighted RMS of d over
 *                               the rows used, the winner's score (NaN without consensus, +inf without a usable hypothesis),
 *                               conditioning (NaN where no fit was tried)}; inlier (n_rows) one flag per row: it entered the fit; dist
 *                               (n_rows) d of every row at the result.  T, scale, RMS and dist are NaN unless the status is OK.
 *   pcs_align_last_kernel_ms    device time of the stages of the last run, kernel_ms[4] = {hypotheses, scores, selection, fit} (no
 *                               counterpart).  PCS_ERR_STATE when the last run had no problems and so queued nothing.
 */
typedef struct pcs_point_aligner pcs_point_aligner;
enum {
    PCS_ALIGN_OK = 0,
    PCS_ALIGN_TOO_FEW = 1,        /* fewer than min_points usable rows */
    PCS_ALIGN_DEGENERATE = 2,     /* conditioning <= rank_tol: collinear or coincident points */
    PCS_ALIGN_NONFINITE = 3,      /* every row has a non-finite coordinate, or the fit overflowed */
    PCS_ALIGN_NO_CONSENSUS = 4    /* enough usable rows, fewer than min_points inliers */
};
enum { PCS_ALIGN_RIGID = 0, PCS_ALIGN_SIMILARITY = 1 };
enum { PCS_ALIGN_OUT_T = 1, PCS_ALIGN_OUT_SCALE = 2, PCS_ALIGN_OUT_INFO = 4, PCS_ALIGN_OUT_STATS = 8, PCS_ALIGN_OUT_INLIER = 16, PCS_ALIGN_OUT_DIST = 32 };
int pcs_align_create(pcs_point_aligner **out, int device);
int pcs_align_destroy(pcs_point_aligner *p);
int pcs_align_set_points(pcs_point_aligner *p, int64_t n_rows, const double *src, const double *dst, const double *weights, int64_t n_problems,
                         const int64_t *start_inds);
int pcs_align_set_consensus(pcs_point_aligner *p, int n_hypotheses, double inlier_dist, uint64_t seed);
int pcs_align_get_consensus(pcs_point_aligner *p, int *n_hypotheses, double *inlier_dist, uint64_t *seed);
int pcs_align_run(pcs_point_aligner *p, int model, int min_points, double rank_tol, int group_lanes, int flags, double *d_T, void *stream);
int pcs_align_results(pcs_point_aligner *p, double *T, double *scale, int32_t *info, double *stats, uint8_t *inlier, double *dist);
int pcs_align_last_kernel_ms(pcs_point_aligner *p, float *kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * A calibration applied to points and images: rays, undistortion and rectified remap (csrc/ba_imagemap.hpp).  Since
 * pcs_version() 122.
 * Replaces: nb_undistort_arr / nb_distort (optimisation/compiled_helpers.py:373-490); sensor_map / vector_cam_points
 *           (utils/general_utils.py:432-483) and Camera._compute_world_sensor_map / im_to_world_ray (cameras/camera.py:162-177, :460-493);
 *           Camera.undistort (cameras/camera.py:451-458) and undistort_im / remap_im / rectify_camera_images
 *           (reconstruction/reconstruction_utils.py:12-107), i.e. cv2.undistort, cv2.initUndistortRectifyMap and cv2.remap.
 * Points, maps and images are DEVICE buffers of the caller, used in place; every call is queued on `stream` (NULL = the handle's stream).
 * All coordinate arithmetic is FP64.  Every argument is checked on the host before the device is touched (PCS_ERR_ARG, or PCS_ERR_STATE
 * for a call that needs cameras or extrinsics that were not set); pcs_last_error names the argument.
 *   pcs_imap_create          a handle on `device` (no counterpart)
 *   pcs_imap_destroy         frees the handle (no counterpart)
 *   pcs_imap_set_cameras     host arrays, copied: intr (n_cams, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2] as for pcs_pnp_set_cameras, finite
 *                            with non-zero focal lengths; ext (n_cams, 12) world -> camera rows [R | t] as for pcs_rigpose_set_extrinsics,
 *                            or NULL (Camera.intrinsic / distortion_coefs / extrinsic).  Resets the view.
 *   pcs_imap_set_view        the new camera of pcs_imap_build_maps and of the fused remap, per camera: R_new (n_cams, 9) row-major, the
 *                            rectifying rotation R of cv2.initUndistortRectifyMap (source camera frame -> new frame), NULL = identity;
 *                            K_new (n_cams, 4) = [fx, cx, fy, cy], NULL = the camera's own, which is cv2.undistort(img, K, d, None, K).
 *   pcs_imap_points          one thread per point.  d_in (n, 2) pixels; d_cam (n) int32 camera per row, or NULL = cam_all for every row; a
 *                            row whose camera lies outside the table gives NaN.  mode PCS_IMAP_UNDISTORT: nb_undistort_arr's fixed point,
 *                            `iters` steps (5 in the reference; 0 .. 100), d_out (n, 2).  PCS_IMAP_DISTORT: nb_distort, d_out (n, 2).
 *                            PCS_IMAP_RAY: vector_cam_points — undistort (unless PCS_IMAP_NO_DISTORT), K^-1, z = 1 or unit length
 *                            (PCS_IMAP_NORMALISED), camera frame or rotated to the world by R_e^T (PCS_IMAP_WORLD), d_out (n, 3).
 *   pcs_imap_rays            sensor_map / world_sensor_map of camera `cam`: every pixel (x, y) of a width x height sensor through the ray
 *                            path, d_out (height, width, 3) in image order, out_dtype PCS_F64 or PCS_F32 (the FP64 result rounded once).
 *                            With d_depth (height, width; depth_dtype PCS_F64 or PCS_F32) the output is position + ray * depth,
 *                            im_to_world_ray(depth_im=) for the whole image (position = 0 in the camera frame); a depth that is not
 *                            finite gives three NaNs.
 *   pcs_imap_build_maps      cv2.initUndistortRectifyMap for camera `cam` and its view: per destination pixel X = R_new^T K_new^-1 (u, v, 1),
 *                            x = X / Z, y = Y / Z, forward distortion, the camera's K; d_out (2, height, width), plane 0 the source x,
 *                            plane 1 the source y, PCS_F32 or PCS_F64.  Z <= 0 gives NaN.
 *   pcs_imap_remap           cv2.remap, batched: n_img (<= 65535) images d_src (n_img, src_height, src_pitch BYTES) -> d_dst (n_img,
 *                            dst_height, dst_pitch BYTES), interleaved channels 1, 3 or 4, dtype PCS_IMAP_U8 or PCS_IMAP_F32.  cams (n_img) is
 *                            a HOST array: the camera of every image.  d_map NULL: FUSED, the coordinate of pcs_imap_build_maps is computed
 *                            in registers and no map is written or read.  Otherwise MAPPED: d_map (n_maps, 2, dst_height, dst_width) of
 *                            map_dtype PCS_F32 or PCS_F64, and image i reads map cams[i].  interpolation: PCS_IMAP_NEAREST (ties to even),
 *                            PCS_IMAP_BILINEAR, PCS_IMAP_BICUBIC (a = -0.75, cv2.INTER_CUBIC).  A tap outside the source takes border[c]
 *                            (border: `channels` host values, NULL = 0; BORDER_CONSTANT); where no tap lies inside, the value is the
 *                            border.  floor, not truncation, for negative coordinates; exact FP64 weights; PCS_IMAP_U8 results are rounded
 *                            half-to-even and saturated (OpenCV's 1/32-pixel weight tables are not reproduced).  d_valid (n_img,
 *                            dst_height, dst_width) uint8 or NULL: 1 where every tap lay inside the source.
 *   pcs_imap_last_kernel_ms  device time of the handle's last launch (no counterpart)
 */
typedef struct pcs_image_mapper pcs_image_mapper;
enum { PCS_IMAP_UNDISTORT = 0, PCS_IMAP_DISTORT = 1, PCS_IMAP_RAY = 2 };
enum { PCS_IMAP_NORMALISED = 1, PCS_IMAP_WORLD = 2, PCS_IMAP_NO_DISTORT = 4 };
enum { PCS_IMAP_NEAREST = 0, PCS_IMAP_BILINEAR = 1, PCS_IMAP_BICUBIC = 2 };
enum { PCS_IMAP_U8 = 0, PCS_IMAP_F32 = 1 };
int pcs_imap_create(pcs_image_mapper **out, int device);
int pcs_imap_destroy(pcs_image_mapper *p);
int pcs_imap_set_cameras(pcs_image_mapper *p, int64_t n_cams, const double *intr, const double *ext);
int pcs_imap_set_view(pcs_image_mapper *p, const double *R_new, const double *K_new);
int pcs_imap_points(pcs_image_mapper *p, int mode, int64_t n, const int32_t *d_cam, int cam_all, const double *d_in, int iters, int flags, double *d_out, void *stream);
int pcs_imap_rays(pcs_image_mapper *p, int cam, int width, int height, int flags, int iters, const void *d_depth, int depth_dtype, void *d_out, int out_dtype, void *stream);
int pcs_imap_build_maps(pcs_image_mapper *p, int cam, int width, int height, void *d_out, int out_dtype, void *stream);
int pcs_imap_remap(pcs_image_mapper *p, int64_t n_img, const int32_t *cams, const void *d_src, int src_width, int src_height, int channels, int dtype, int64_t src_pitch,
                   void *d_dst, int dst_width, int dst_height, int64_t dst_pitch, const void *d_map, int map_dtype, int64_t n_maps, int interpolation, const double *border,
                   uint8_t *d_valid, void *stream);
int pcs_imap_last_kernel_ms(pcs_image_mapper *p, float *kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Dense stereo on a rectified pair: block matching, disparity to points, compaction (csrc/ba_stereo.hpp).  Since
 * pcs_version() 123.
 * Replaces: the second half of stereo_reconstruct (reconstruction/reconstruction_utils.py:170-223): cv2.StereoBM_create(...).compute / 16,
 *           cv2.reprojectImageTo3D, and the NaN / inf / depth mask of depth_image_ptcloud_mask (:24-38) and disparity_to_ptcld (:110-137)
 *           with the masked cloud and the left image's grey value per point.
 * OpenCV's StereoBM is NOT reproduced bit for bit (its NORMALIZED_RESPONSE prefilter, its SIMD rounding and its dispDescale are its own).
 * The rule is all integers: two runs, and any tiling, give the same bits.  tests/stereo_reference.py states it in NumPy.
 *   prefilter (cap > 0)  P = clip(g, -cap, cap) + cap, g the 3 x 3 horizontal Sobel response with the rows clamped; columns 0 and W - 1
 *                        are cap.  cap = 0: P = I (texture_threshold must then be 0).
 *   cost                 C(y, x, d) = sum over the block x block window of |P_L(y + j, x + i) - P_R(y + j, x + i - d)|, d = u_L - u_R in
 *                        [min_disp, min_disp + num_disp - 1]; defined where both windows lie inside the image.
 *   strict pixels        a left pixel competes only if C is defined for every d of the range; every other pixel has PCS_STEREO_NOT_STRICT.
 *   winner               d* the smallest d of the smallest cost C*.
 *   PCS_STEREO_TEXTURE   (cap > 0) sum over the window of |P_L - cap| < texture_threshold.
 *   PCS_STEREO_UNIQUENESS  (uniqueness_ratio u > 0) some d with |d - d*| >= 2 has 100 C(d) <= (100 + u) C*.
 *   PCS_STEREO_LEFT_RIGHT  (lr_max_diff >= 0) |d* - d_R(y, x - d*)| > lr_max_diff, d_R the winner anchored in the right image over the d
 *                        for which the cost is defined (the range is clamped per pixel).
 *   PCS_STEREO_VALIDITY  (validity planes) valid_left(y, x) = 0 or valid_right(y, x - d*) = 0.
 *   sub-pixel            m = C(d* - 1), p = C(d* + 1), den = 2 (m + p - 2 C*); 0 when d* is an end of the range or den = 0, else
 *                        floor((32 (m - p) + den) / (2 den)): 16 (m - p) / den rounded half up, in [-8, 8].
 *   pcs_stereo_create    a handle on `device` (no counterpart); it owns the workspace: the two prefiltered planes, the right-anchored
 *                        disparity and the compaction's counts, O(n width height) bytes — the cost volume is never stored
 *   pcs_stereo_destroy   frees the handle (no counterpart)
 *   pcs_stereo_match     StereoBM.compute over n (<= 32767) pairs: d_left / d_right (n, height, pitch BYTES) 8-bit single channel;
 *                        min_disp in [-1024, 1024], num_disp in [1, 1024], block odd in [3, 31], prefilter_cap in [0, 63],
 *                        texture_threshold >= 0, uniqueness_ratio in [0, 100], lr_max_diff >= -1 (-1: no left-right pass);
 *                        d_valid_left / d_valid_right (n, height, width) uint8 or both NULL.  d_disp (n, height, width) int16 = 16 d* +
 *                        offset where the status is 0 and 16 (min_disp - 1) elsewhere (cv2's convention); d_cost int32 or NULL: C* on
 *                        strict pixels, -1 elsewhere; d_status uint8 or NULL: the bits above, each evaluated on every strict pixel.
 *   pcs_stereo_reproject cv2.reprojectImageTo3D and the reference's mask: (X, Y, Z, Wh) = Q (x, y, disp / 16, 1) in FP64, point =
 *                        (X, Y, Z) / Wh.  Q: HOST (n_Q, 16) row-major, n_Q = 1 (one for all) or n.  mask = disp != invalid_disp (a value
 *                        outside int16: every disparity counts) and all three coordinates finite and z_lo <= z <= z_hi (-inf / +inf: no
 *                        bound).  T: HOST 3 x 4 rigid transform applied to the masked points (the z of the mask is the one before it), or
 *                        NULL.  d_points (n, height, width, 3) of dtype PCS_F64 or PCS_F32 (the FP64 result rounded once), three NaNs where
 *                        the mask is 0; d_mask (n, height, width) uint8; d_counts (n) int64 on the DEVICE or NULL: the mask's sum per pair.
 *   pcs_stereo_compact   the masked cloud: the points with mask != 0 of pair 0, then pair 1, ..., each in row-major pixel order, packed into
 *                        d_out_points (room for every pixel), with d_values (n, height, values_pitch BYTES; the left image) into d_out_values
 *                        (both or neither); d_counts (n) int64 on the DEVICE.  Stable, without atomics.
 *   pcs_stereo_last_kernel_ms  device time of the handle's last call (no counterpart)
 * Every argument is checked on the host before the device is touched (PCS_ERR_ARG; pcs_last_error names the argument); the handle is
 * looked at last.  All buffers are DEVICE buffers of the caller unless marked HOST; calls are queued on `stream` (NULL = the handle's).
 */
typedef struct pcs_stereo_matcher pcs_stereo_matcher;
enum { PCS_STEREO_NOT_STRICT = 1, PCS_STEREO_TEXTURE = 2, PCS_STEREO_UNIQUENESS = 4, PCS_STEREO_LEFT_RIGHT = 8, PCS_STEREO_VALIDITY = 16 };
int pcs_stereo_create(pcs_stereo_matcher **out, int device);
int pcs_stereo_destroy(pcs_stereo_matcher *p);
int pcs_stereo_match(pcs_stereo_matcher *p, int64_t n, int width, int height, const uint8_t *d_left, int64_t left_pitch, const uint8_t *d_right, int64_t right_pitch, int min_disp,
                     int num_disp, int block, int prefilter_cap, int texture_threshold, int uniqueness_ratio, int lr_max_diff, const uint8_t *d_valid_left,
                     const uint8_t *d_valid_right, int16_t *d_disp, int32_t *d_cost, uint8_t *d_status, void *stream);
int pcs_stereo_reproject(pcs_stereo_matcher *p, int64_t n, int width, int height, const int16_t *d_disp, int invalid_disp, const double *Q, int64_t n_Q, double z_lo, double z_hi,
                         const double *T, void *d_points, int dtype, uint8_t *d_mask, int64_t *d_counts, void *stream);
int pcs_stereo_compact(pcs_stereo_matcher *p, int64_t n, int width, int height, const void *d_points, int dtype, const uint8_t *d_mask, const uint8_t *d_values,
                       int64_t values_pitch, void *d_out_points, uint8_t *d_out_values, int64_t *d_counts, void *stream);
int pcs_stereo_last_kernel_ms(pcs_stereo_matcher *p, float *kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * Semi-global matching on a rectified pair: census cost, 4 / 8-path aggregation (csrc/ba_stereo_sgm.hpp).  Since
 * pcs_version() 124.
 * Replaces: matlab_stereo (reconstruction/reconstruction_utils.py:140-167), the matlab=True branch of stereo_reconstruct, which starts a
 *           MATLAB engine per call for disparitySGM(im0, im1, 'DisparityRange', ..., 'UniquenessThreshold', ...).
 * Neither MATLAB's disparitySGM nor OpenCV's StereoSGBM is reproduced bit for bit.  The rule is all integers: two runs, any order of the
 * directions and any chunking of the batch give the same bits.  tests/sgm_reference.py states it in NumPy.  Handle, status bits, the
 * int16 disparity in sixteenths, pcs_stereo_reproject and pcs_stereo_compact are those of the block matcher above.  There is no
 * prefilter: the census runs on the raw bytes.
 *   census               window census_w x census_h (both odd, >= 3, census_w census_h - 1 <= 64), rw = census_w / 2, rh = census_h / 2.
 *                        The descriptor of a pixel whose window lies inside the image has one bit per window position other than the
 *                        centre: 1 iff that neighbour is LESS THAN the centre.
 *   cost                 C(y, x, d) = popcount(c_L(y, x) xor c_R(y, x - d)), d = u_L - u_R in [min_disp, min_disp + num_disp - 1], defined
 *                        where both windows lie inside their images; 0 <= C <= 64.
 *   strict pixels        a left pixel competes only if C is defined for every d of the range: rows rh .. H - 1 - rh, columns
 *                        rw + max(d_max, 0) .. W - 1 - rw + min(min_disp, 0).  Every other pixel has PCS_STEREO_NOT_STRICT, disparity
 *                        16 (min_disp - 1) and cost -1.  An empty rectangle is a valid call.
 *   aggregation          directions r = (0, +-1), (+-1, 0) (paths = 4) and (+-1, +-1) (paths = 8).  At a strict pixel p: if p - r is not
 *                        strict the path starts here, L_r(p, d) = C(p, d); else, with M = min_j L_r(p - r, j),
 *                        L_r(p, d) = C(p, d) + min(L_r(p - r, d), L_r(p - r, d - 1) + P1, L_r(p - r, d + 1) + P1, M + P2) - M,
 *                        a term whose disparity leaves the range omitted.  S(p, d) = sum over r of L_r(p, d).  0 <= P1 <= P2 <= 1023,
 *                        so L_r <= 64 + P2 <= 1087 and S <= 8 * 1087 < 2^14: S is held in 16 bits.
 *   winner               d* the smallest d of the smallest S; cost = S(d*).
 *   PCS_STEREO_UNIQUENESS  (uniqueness_ratio u > 0) some d with |d - d*| >= 2 has 100 S(d) <= (100 + u) S*.
 *   PCS_STEREO_LEFT_RIGHT  (lr_max_diff >= 0) |d* - d_R(y, x - d*)| > lr_max_diff, d_R(y, x2) the smallest d minimising S(y, x2 + d, d) over
 *                        the d for which (y, x2 + d) is strict: read from the SAME S, there is no second aggregation.
 *   PCS_STEREO_VALIDITY  as above.  PCS_STEREO_TEXTURE is never set: a census has no texture measure.
 *   sub-pixel            the block matcher's floor division on S(d* - 1), S*, S(d* + 1).
 *   pcs_stereo_sgm       over n (<= 32767) pairs; min_disp in [-1024, 1024], num_disp in [1, 256], p1 / p2 the penalties, paths 4 or 8,
 *                        uniqueness_ratio in [0, 100], lr_max_diff >= -1; images, validity planes and the three outputs as in
 *                        pcs_stereo_match.  The matching-cost volume is never stored; S (2 height width Dpad bytes per pair, Dpad =
 *                        num_disp rounded up to 4) and the census planes (16 height width bytes per pair) are workspace of the handle,
 *                        and the batch is walked in chunks of pairs that fit the workspace limit.
 *   pcs_stereo_set_sgm_workspace  the limit in bytes (0: the default, 16 GiB).  pcs_stereo_sgm answers a limit below one pair's need with
 *                        PCS_ERR_ARG and the needed byte count in pcs_last_error().  Chunking does not change a bit of the output.
 * Every argument is checked on the host before the device is touched; the handle is looked at last.
 */
int pcs_stereo_sgm(pcs_stereo_matcher *p, int64_t n, int width, int height, const uint8_t *d_left, int64_t left_pitch, const uint8_t *d_right, int64_t right_pitch, int min_disp,
                   int num_disp, int census_w, int census_h, int p1, int p2, int paths, int uniqueness_ratio, int lr_max_diff, const uint8_t *d_valid_left,
                   const uint8_t *d_valid_right, int16_t *d_disp, int32_t *d_cost, uint8_t *d_status, void *stream);
int pcs_stereo_set_sgm_workspace(pcs_stereo_matcher *p, int64_t bytes);

/* ------------------------------------------------------------------------------------------------
 * Depth-map fusion across views: geometric consistency filter and merged cloud (csrc/ba_fusion.hpp).  Since
 * pcs_version() 125.
 * Replaces: the step the reference leaves to an external multi-view program.  It writes the rig out (CameraSet.write_to_txt,
 *           cameras/camera_set.py:235-272; Camera.to_MVSnet_txt, cameras/camera.py:130-160; calc_pairs / write_pair_file,
 *           reconstruction/acmmp_utils.py:24-83) and reads that program's fused cloud back.  What the program adds over per-view depth maps
 *           is the geometric consistency check and fusion of MVSNet (filter_depth) / ACMMP / COLMAP; the rule below is the library's own,
 *           in that spirit.  tests/fusion_reference.py states it in NumPy.
 * Inputs.  V views of one size W x H.  View v is a DISTORTION-FREE pinhole, K_v = [fx, cx, fy, cy] and [R_v | t_v] world -> view: the maps
 * are those of undistorted or rectified images (pixel (x, y) is the ray ((x - cx) / fx, (y - cy) / fy, 1)).  D_v (H, W) is a z-depth map,
 * float32 or float64; a depth is INVALID when it is NaN, +-inf or <= 0.  Every view has an ordered neighbour list in CSR form (nbr_start
 * (V + 1), nbr, int32) of at most 32 views, never itself, none twice.  Scalars px_tol > 0, rel_tol > 0, min_views in [1, 32].
 * The rule.  All arithmetic is FP64, plain IEEE operations in the order written (no contraction), sums of three products taken left to
 * right.  For the reference pixel (i, x, y) with valid z = D_i[y, x]:
 *   1. back-projection   c = (z ((x - cx_i) / fx_i) - t_i0, z ((y - cy_i) / fy_i) - t_i1, z - t_i2), X = R_i^T c.
 *   2. each neighbour j in list order is CONSISTENT when none of these fails (a comparison with a NaN fails):
 *        Y = R_j X + t_j; fail unless Y_z > 0.
 *        (u, v) = (fx_j (Y_x / Y_z) + cx_j, fy_j (Y_y / Y_z) + cy_j), q = (floor(u + 0.5), floor(v + 0.5)); fail unless q lies in
 *        [0, W) x [0, H).
 *        z_j = D_j[q]; fail if z_j is invalid.
 *        X_j = the back-projection of q at z_j in view j (step 1 with j's parameters); Y' = R_i X_j + t_i; fail unless Y'_z > 0.
 *        (x', y') = the projection of Y' by K_i; fail unless (x' - x)^2 + (y' - y)^2 <= px_tol^2 and |Y'_z - z| <= rel_tol z.
 *   3. support (uint32) has bit k set when the k-th neighbour of the list is consistent; count = popcount(support); the pixel is KEPT
 *      iff count >= min_views.
 *   4. fused point F = (X + sum of X_j over the consistent neighbours, in list order) / (count + 1), each coordinate divided.  With T
 *      (3 x 4, rigid) the point written is T (F, 1); it is rounded once to float32 or left as float64, and is three NaNs where the pixel
 *      is not in the mask.  fused_depth = the z of the UNTRANSFORMED F in view i, (R_i F + t_i)_z, NaN where the pixel is not in the mask.
 *   5. unique (opt-in): a kept pixel (i, x, y) is a DUPLICATE when, for some consistent neighbour j with j < i, the partner pixel q of
 *      step 2 is itself kept by step 3 — kept BEFORE any duplicate marking, so the result does not depend on an order of evaluation.
 *      Duplicates leave the mask: the lowest view owns a surface element.
 *   6. status (uint8): PCS_FUSE_INVALID_DEPTH (the input depth is invalid; steps 1 to 5 are not taken and support = count = 0),
 *      PCS_FUSE_FEW_VIEWS (a valid depth with count < min_views), PCS_FUSE_DUPLICATE.  mask = 1 iff status = 0.
 * No atomics; two runs give identical bits.
 *   pcs_fuse_create          a handle on `device` (no counterpart); it owns the view table, the neighbour lists and the workspace (the
 *                            4-byte support word per pixel when the caller does not ask for it, and the block counts of d_counts)
 *   pcs_fuse_destroy         frees the handle (no counterpart)
 *   pcs_fuse_set_views       what write_to_txt / to_MVSnet_txt hand to the external program: the intrinsics and extrinsics of every
 *                            view.  n_views in [1, 32767] (the compaction's limit), width and height in [1, 65535]; K HOST (n_views, 4),
 *                            P HOST (n_views, 12) = [R | t] row-major; both are copied.  Finite, fx and fy != 0.  New views drop the
 *                            neighbour lists.
 *   pcs_fuse_set_neighbours  what write_pair_file hands over: HOST CSR lists for the n = n_views views.  nbr_start runs from 0 and never
 *                            decreases, at most 32 entries per view, every index in [0, n), no view its own neighbour, none twice.
 *   pcs_fuse_run             the external program's consistency filter and fusion.  d_depth (n_views, height, width) of depth_dtype;
 *                            unique 0 or 1; T HOST 3 x 4 or NULL; d_points (n_views, height, width, 3) of points_dtype; d_mask uint8.
 *                            Optional (NULL: not written): d_count uint8, d_support uint32, d_status uint8, d_fused_depth of fused_dtype
 *                            (all (n_views, height, width)) and d_counts (n_views) int64 on the DEVICE, the mask's sum per view as
 *                            pcs_stereo_reproject fills it, so that pcs_stereo_compact can follow unchanged.  dtypes: PCS_F64 or PCS_F32.
 *                            Two launches: the check of every view, then (unique) the duplicate marking, which reads the support words.
 *   pcs_fuse_last_kernel_ms  device time of the last run (no counterpart): the check kernel, the duplicate kernel (0 without unique) and
 *                            the whole call, the counts included
 * Every argument is checked on the host before the device is touched (PCS_ERR_ARG; pcs_last_error names the argument); the handle is
 * looked at last.  All buffers are DEVICE buffers of the caller unless marked HOST; a run is queued on `stream` (NULL = the handle's).
 */
typedef struct pcs_depth_fuser pcs_depth_fuser;
enum { PCS_FUSE_INVALID_DEPTH = 1, PCS_FUSE_FEW_VIEWS = 2, PCS_FUSE_DUPLICATE = 4, PCS_FUSE_MAX_NEIGHBOURS = 32 };
int pcs_fuse_create(pcs_depth_fuser **out, int device);
int pcs_fuse_destroy(pcs_depth_fuser *p);
int pcs_fuse_set_views(pcs_depth_fuser *p, int64_t n_views, int width, int height, const double *K, const double *P);
int pcs_fuse_set_neighbours(pcs_depth_fuser *p, const int32_t *nbr_start, const int32_t *nbr, int64_t n);
int pcs_fuse_run(pcs_depth_fuser *p, const void *d_depth, int depth_dtype, double px_tol, double rel_tol, int min_views, int unique, const double *T, void *d_points,
                 int points_dtype, uint8_t *d_mask, uint8_t *d_count, uint32_t *d_support, uint8_t *d_status, void *d_fused_depth, int fused_dtype, int64_t *d_counts,
                 void *stream);
int pcs_fuse_last_kernel_ms(pcs_depth_fuser *p, float *check_ms, float *unique_ms, float *total_ms);

/* ------------------------------------------------------------------------------------------------
 * Plane-sweep multi-view depth: from the images of a rig to one z-depth map per view (csrc/ba_sweep.hpp).  Since
 * pcs_version() 126.
 * Replaces: the depth estimation of the external multi-view program the reference writes its rig out for.  What the reference hands
 *           over is a rig, per-view neighbour lists of up to nine views and a depth range cut into steps: ReconParams(mindist, maxdist,
 *           steps = 192, max_n_view = 9) (reconstruction/acmmp_utils.py:6-21), the last line Camera.to_MVSnet_txt writes, `depth_min
 *           interval steps depth_max` (cameras/camera.py:158-159), and calc_pairs.  Those are the inputs of a plane sweep.  Neither
 *           MVSNet nor ACMMP is reproduced: the rule below is the library's own.  tests/sweep_reference.py states it in NumPy.
 * Inputs.  V views of one size W x H, 8-bit single-channel images I_v (V, H, pitch BYTES).  View v is a DISTORTION-FREE pinhole,
 * K_v = [fx, cx, fy, cy] and [R_v | t_v] world -> view (the conventions of pcs_fuse_set_views); ordered neighbour lists in CSR form as
 * in pcs_fuse_set_neighbours, at most PCS_SWEEP_MAX_NEIGHBOURS = 16 per view.  A HOST table of plane depths z (n_z, D) float64, n_z = 1
 * (one row for all views) or V, D in [1, PCS_SWEEP_MAX_PLANES = 1024], every z finite and > 0, strictly monotone along a row.  Census
 * window cw x ch (the limits of pcs_stereo_sgm), rw = cw / 2, rh = ch / 2; box radius r in [0, 4]; truncate tau in
 * [1, (cw ch - 1)(2 r + 1)^2]; uniqueness_ratio u in [0, 100].
 * The rule, for reference view i, pixel p = (x, y), plane k and neighbour j of i's list:
 *   1. warp.  The host forms, in FP64, plain operations in the order written, sums of three products left to right:
 *        M = R_j R_i^T, c = t_j - M t_i; N = K_j M, i.e. N_0. = fx_j M_0. + cx_j M_2., N_1. = fy_j M_1. + cy_j M_2., N_2. = M_2.;
 *        A_a0 = N_a0 / fx_i, A_a1 = N_a1 / fy_i, A_a2 = (N_a2 - A_a0 cx_i) - A_a1 cy_i   (A = K_j M K_i^-1);
 *        b = K_j c = (fx_j c_0 + cx_j c_2, fy_j c_1 + cy_j c_2, c_2).
 *      The device reads these 12 numbers and computes, in FP64, plain IEEE operations in the order written, no contraction:
 *        n_a = z_k ((A_a0 x + A_a1 y) + A_a2) + b_a for a = 0, 1, 2; u = n_0 / n_2, v = n_1 / n_2.
 *   2. sample (integers from here on).  q_u = floor(16 u + 0.5), q_v = floor(16 v + 0.5): the nearest sixteenth.  The sample is VALID
 *      iff n_2 > 0, 0 <= q_u < 16 (W - 1) and 0 <= q_v < 16 (H - 1) (a comparison with a NaN fails).  x0 = q_u >> 4, f_x = q_u & 15,
 *      likewise y0, f_y; g = (16 - f_x)(16 - f_y) I_j[y0, x0] + f_x (16 - f_y) I_j[y0, x0 + 1] + (16 - f_x) f_y I_j[y0 + 1, x0]
 *      + f_x f_y I_j[y0 + 1, x0 + 1], in [0, 65280].
 *   3. cost per neighbour.  W_jk(p) = g at reference pixel p.  Its census descriptor is that of pcs_stereo_sgm (one bit per window
 *      position other than the centre, 1 iff that neighbour is LESS THAN the centre) and is valid iff every sample of the window is
 *      valid; the reference descriptor is the census of I_i.  h(p, k, j) = popcount of the xor of the two.
 *      C_j(p, k) = min(tau, sum of h(q, k, j) over the (2 r + 1)^2 box about p), and tau outright when a descriptor of the box is
 *      invalid: occluded, out-of-view and behind-the-camera neighbours all cost tau.
 *   4. merge.  C(p, k) = sum over the list of C_j(p, k): an integer, so the order of a list does not change a bit.  STRICT pixels are
 *      those whose box and census footprint lies inside the reference image: rows rh + r .. H - 1 - rh - r, columns rw + r ..
 *      W - 1 - rw - r.  An empty rectangle is a valid call.
 *   5. decide.  k* the smallest k of the smallest C; cost = C* = C(p, k*).  Offset f: the block matcher's floor division (above,
 *      "sub-pixel") on C(k* - 1), C*, C(k* + 1), 0 when k* is an end of the table.  level = 16 k* + f (int32).  status (uint8), the
 *      first that applies set alone: PCS_SWEEP_NOT_STRICT; PCS_SWEEP_NO_VIEW: C* >= tau (list length), no neighbour scored below the
 *      truncation at any plane (an empty list gives it on every strict pixel); PCS_SWEEP_UNIQUENESS: u > 0 and some k with
 *      |k - k*| >= 2 has 100 C(k) <= (100 + u) C*.  depth = z[k*] + (|f| / 16)(z[k* + sign f] - z[k*]) in FP64 in that order, rounded
 *      once for a float32 output, NaN wherever status != 0.  Non-strict pixels have level -16 and cost -1; level and cost of a strict
 *      pixel are written whatever its status.
 * No atomics; two runs, any tiling and any order of a neighbour list give identical bits.  The cost volume is never stored.
 *   pcs_sweep_create          a handle on `device` (no counterpart); it owns the neighbour lists, the warp table and the plane table
 *   pcs_sweep_destroy         frees the handle (no counterpart)
 *   pcs_sweep_set_views       arguments and checks of pcs_fuse_set_views.  New views drop the neighbour lists.
 *   pcs_sweep_set_neighbours  arguments and checks of pcs_fuse_set_neighbours, with at most 16 entries per view
 *   pcs_sweep_run             d_images (n_views, height, pitch BYTES); z HOST (n_z, D); d_depth (n_views, height, width) of depth_dtype
 *                             PCS_F64 or PCS_F32.  Optional (NULL: not written): d_level int32, d_cost int32, d_status uint8.
 *   pcs_sweep_last_kernel_ms  device time of the last run's kernel (no counterpart)
 * Every argument is checked on the host before the device is touched (PCS_ERR_ARG; pcs_last_error names the argument); the handle is
 * looked at last, and with it n_z against the views and pitch against the width.  All buffers are DEVICE buffers of the caller unless
 * marked HOST; a run is queued on `stream` (NULL = the handle's).
 */
typedef struct pcs_plane_sweeper pcs_plane_sweeper;
enum { PCS_SWEEP_NOT_STRICT = 1, PCS_SWEEP_NO_VIEW = 2, PCS_SWEEP_UNIQUENESS = 4, PCS_SWEEP_MAX_NEIGHBOURS = 16, PCS_SWEEP_MAX_PLANES = 1024 };
int pcs_sweep_create(pcs_plane_sweeper **out, int device);
int pcs_sweep_destroy(pcs_plane_sweeper *p);
int pcs_sweep_set_views(pcs_plane_sweeper *p, int64_t n_views, int width, int height, const double *K, const double *P);
int pcs_sweep_set_neighbours(pcs_plane_sweeper *p, const int32_t *nbr_start, const int32_t *nbr, int64_t n);
int pcs_sweep_run(pcs_plane_sweeper *p, const uint8_t *d_images, int64_t pitch, const double *z, int64_t n_z, int D, int census_w, int census_h, int box_radius, int truncate,
                  int uniqueness_ratio, void *d_depth, int depth_dtype, int32_t *d_level, int32_t *d_cost, uint8_t *d_status, void *stream);
int pcs_sweep_last_kernel_ms(pcs_plane_sweeper *p, float *kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * PatchMatch multi-view depth: a slanted plane per pixel, spread between pixels and refined at random (SURVEY 8 row f20;
 * csrc/ba_patchmatch.hpp).  Since pcs_version() 130.
 * Replaces: what the plane sweep above cannot give of the external program the reference exports its rig for (ACMMP is a PatchMatch
 *           method: reconstruction/acmmp_utils.py, ReconParams, Camera.to_MVSnet_txt): unbiased depth on surfaces seen obliquely, depth
 *           finer than a plane table, and a normal per pixel.  ACMMP is not reproduced: the rule below is the library's own, designed so
 *           that the device can be held to equality.  tests/patchmatch_reference.py states it in NumPy.
 * Inputs.  Views, images, intrinsics, extrinsics and neighbour lists are those of pcs_sweep_set_views / pcs_sweep_set_neighbours (at
 * most PCS_PM_MAX_NEIGHBOURS = 16 per view).  A HOST table wrange (n_w, 2) float64, n_w = 1 or V, of inverse-depth bounds [w_lo, w_hi],
 * 0 < w_lo < w_hi, both finite.  Census window cw x ch (the limits of pcs_stereo_sgm), rw = cw / 2, rh = ch / 2, and a window stride s
 * in [1, 4]: the footprint is ((cw - 1) s + 1) x ((ch - 1) s + 1).  truncate tau in [1, cw ch - 1].  slope_max sigma (V doubles, > 0,
 * finite, HOST): tan(largest slant) / min(fx, fy).  seed (uint64).
 * State.  Per pixel of every view a plane (w, a, b) in float64 — w the inverse z-depth AT the pixel, a and b its change per pixel in x
 * and y: the inverse depth of a plane is exactly affine in the pixel coordinates of a pinhole view — and an int32 cost.  STRICT pixels
 * are those whose footprint lies inside the image: rows rh s .. H - 1 - rh s, columns rw s .. W - 1 - rw s; an empty rectangle is a valid
 * call.  A non-strict pixel holds the plane (NaN, NaN, NaN) and cost -1.
 * Admissible.  A plane is admissible at a pixel of view i iff w_lo <= w <= w_hi, |a| <= sigma_i w and |b| <= sigma_i w, in plain FP64 (the
 * product first), a comparison with a NaN failing.
 * Cost C of plane (w, a, b) at strict pixel p = (x, y) of view i:
 *   1. for neighbour j the 12 numbers A, b of the sweep's step 1, formed by the same host code.
 *   2. for window position (dx, dy), dx in -rw .. rw, dy in -rh .. rh, in FP64, plain IEEE operations in the order written, no
 *      contraction: x' = x + s dx, y' = y + s dy (integers); omega = (w + a (s dx)) + b (s dy);
 *      n_c = ((A_c0 x' + A_c1 y') + A_c2) + omega b_c for c = 0, 1, 2; u = n_0 / n_2, v = n_1 / n_2.
 *   3. the sample is VALID iff omega > 0, n_2 > 0 and the sweep's step-2 range test passes on q_u = floor(16 u + 0.5),
 *      q_v = floor(16 v + 0.5); g is the sweep's integer bilinear value in [0, 65280].
 *   4. the descriptor has one bit per window position other than the centre, 1 iff g(dx, dy) < g(0, 0); it is valid iff every sample is.
 *   5. the reference descriptor is the same census of I_i at the strided positions: I_i[y', x'] < I_i[y, x].
 *   6. h_j = popcount of the xor of the two;  7. C_j = min(tau, h_j) when the descriptor is valid, tau outright when it is not;
 *   8. C = sum over the list of C_j: an integer, so the order of a list does not change a bit.
 * Random numbers: the generator of csrc/ba_consensus.hpp (mix = its splitmix64 finaliser, G = 0x9e3779b97f4a7c15), t the step counter:
 *   k = mix(seed + G); k = mix(k ^ view); k = mix(k ^ (y W + x)); k = mix(k ^ t); r_d = double(mix(k + (d + 1) G) >> 11) 2^-53 in [0, 1).
 *   A DRAW from (r_d, r_d+1, r_d+2) is w = w_lo + r_d (w_hi - w_lo), a = (sigma w)(2 r_d+1 - 1), b = (sigma w)(2 r_d+2 - 1).
 * Initialise (t = 0; pcs_pm_init), every strict pixel: with a start depth map whose value d is valid (finite, > 0) the plane is
 *   (clamp(1 / d, w_lo, w_hi), 0, 0); with start_planes = 1 the plane d_plane holds, where it is admissible; otherwise the draw from
 *   (r_0, r_1, r_2).  cost = C of that plane (a start plane's cost is recomputed).
 * Iterate (pcs_pm_iterate).  Iteration `it` (absolute, 0-based, at most 1000) runs colour c = 0, then c = 1; the colour of a pixel is
 *   (x + y) & 1 and the half-iteration has t = 1 + 2 it + c.  Only strict pixels of colour c change, and they read only pixels of the
 *   other colour, as those stood before the half-iteration.  Each tries these candidates in order; a candidate replaces the current
 *   plane and cost iff it is admissible and its C is strictly less than the current cost:
 *     propagation from the pixels at (ox, oy) = (-1, 0), (1, 0), (0, -1), (0, 1), (-5, 0), (5, 0), (0, -5), (0, 5), skipping a source that
 *       is not strict: for its plane (w_q, a_q, b_q) the candidate is ((w_q - a_q ox) - b_q oy, a_q, b_q), the same plane read at p;
 *     perturbation of the then-current plane (w, a, b), with rho = 2^-(2 + it) and delta = (sigma w) 2^-(1 + it):
 *       A (w (1 + rho (2 r_0 - 1)), a, b);  B (w, a + delta (2 r_1 - 1), b + delta (2 r_2 - 1));
 *       C (w (1 + rho (2 r_3 - 1)), a + delta (2 r_4 - 1), b + delta (2 r_5 - 1));  D the draw from (r_6, r_7, r_8),
 *       each of B, C and D starting from whatever plane is current when its turn comes.
 * Finish (pcs_pm_finish).  status (uint8), the first that applies: PCS_PM_NOT_STRICT; PCS_PM_NO_VIEW: cost >= tau (list length) (an empty
 *   list gives it on every strict pixel).  depth = 1 / w, rounded once for a float32 output, NaN where status != 0.  normal, in the view's
 *   camera frame, unit length, facing the camera: m = (a fx, b fy, (w + a (cx - x)) + b (cy - y)), normal = -m / sqrt((m_0^2 + m_1^2) +
 *   m_2^2), of the depth's dtype, NaN where status != 0.
 * No atomics.  A half-iteration depends only on the state before it: any tiling, a second run and any order of a neighbour list give
 * identical bits, and iterations 0 .. n - 1 in one call equal any split of them over calls.
 *   pcs_pm_create / pcs_pm_destroy / pcs_pm_set_views / pcs_pm_set_neighbours   as their pcs_sweep_* counterparts
 *   pcs_pm_init            d_images (n_views, height, pitch BYTES); d_start_depth (n_views, height, width) of start_dtype or NULL;
 *                          start_planes 0 or 1 (not with a start depth); d_plane (n_views, height, width, 3) float64 and d_cost
 *                          (n_views, height, width) int32 are written (d_plane is read first when start_planes = 1)
 *   pcs_pm_iterate         iterations first_iteration .. first_iteration + n_iterations - 1 on d_plane and d_cost in place
 *   pcs_pm_finish          d_depth (n_views, height, width) of depth_dtype; optional (NULL: not written) d_normal (n_views, height,
 *                          width, 3) of depth_dtype and d_status uint8.  It reads the tables of the last pcs_pm_init or pcs_pm_iterate.
 *   pcs_pm_last_kernel_ms  device time of the last call's kernels
 * Every argument is checked on the host before the device is touched (PCS_ERR_ARG; pcs_last_error names the argument); the handle is
 * looked at last.  All buffers are DEVICE buffers of the caller unless marked HOST; a call is queued on `stream` (NULL = the handle's).
 */
typedef struct pcs_patchmatch pcs_patchmatch;
enum { PCS_PM_NOT_STRICT = 1, PCS_PM_NO_VIEW = 2, PCS_PM_MAX_NEIGHBOURS = 16 };
int pcs_pm_create(pcs_patchmatch **out, int device);
int pcs_pm_destroy(pcs_patchmatch *p);
int pcs_pm_set_views(pcs_patchmatch *p, int64_t n_views, int width, int height, const double *K, const double *P);
int pcs_pm_set_neighbours(pcs_patchmatch *p, const int32_t *nbr_start, const int32_t *nbr, int64_t n);
int pcs_pm_init(pcs_patchmatch *p, const uint8_t *d_images, int64_t pitch, const double *wrange, int64_t n_w, const double *slope_max, int census_w, int census_h, int stride,
                int truncate, uint64_t seed, const void *d_start_depth, int start_dtype, int start_planes, double *d_plane, int32_t *d_cost, void *stream);
int pcs_pm_iterate(pcs_patchmatch *p, int first_iteration, int n_iterations, const uint8_t *d_images, int64_t pitch, const double *wrange, int64_t n_w, const double *slope_max,
                   int census_w, int census_h, int stride, int truncate, uint64_t seed, double *d_plane, int32_t *d_cost, void *stream);
int pcs_pm_finish(pcs_patchmatch *p, int census_w, int census_h, int stride, int truncate, const double *d_plane, const int32_t *d_cost, void *d_depth, int depth_dtype,
                  void *d_normal, uint8_t *d_status, void *stream);
int pcs_pm_last_kernel_ms(pcs_patchmatch *p, float *kernel_ms);

/* ------------------------------------------------------------------------------------------------
 * TSDF volume and surface extraction: from z-depth maps to a quad mesh (csrc/ba_tsdf.hpp).  Since pcs_version() 127.
 * Replaces: nothing the reference computes.  It draws everything as pyvista meshes, and leaves the step from views to a surface to the
 *           external multi-view program and to whatever mesher the user runs on that program's cloud.  The depth maps of pcs_sweep_run /
 *           pcs_stereo_* are what a volumetric fusion needs; it adds what pcs_fuse_run cannot give: free-space carving (a wrong depth in
 *           one view is out-voted by the views that see through it) and a connected surface.  The volume is Curless and Levoy's truncated
 *           signed distance with unit weights; the mesh is naive surface nets (Gibson), which need no case table.  The rule below is the
 *           library's own; tests/tsdf_reference.py states it in NumPy.
 * Inputs.  Views, intrinsics, extrinsics, depth maps and the validity of a depth are those of pcs_fuse_set_views / pcs_fuse_run:
 * distortion-free pinholes K = [fx, cx, fy, cy], [R | t] world -> view, z-depth float32 or float64, invalid when NaN, +-inf or <= 0.
 * All arithmetic is FP64, plain IEEE operations in the order written (no contraction), sums of three products taken left to right.
 * Grid.  Origin o (3 doubles), voxel size s > 0, node counts (nx, ny, nz), each in [1, PCS_TSDF_MAX_DIM = 1024].  Node (i, j, k) is the
 * world point X = (o0 + s i, o1 + s j, o2 + s k); its linear index is (k ny + j) nx + i, taken in int64_t.  Per node the volume holds sum
 * (float32 by default, float64 opt-in) and weight (uint16), both 0 at the start.
 * Integration of an ordered list of views v_0 .. v_{m-1} (indices into the view table; the default is all views in order), trunc > 0.
 * For each node, S = double(sum), W = weight, and for each view of the list in order:
 *   1. Y_a = ((R_a0 X0 + R_a1 X1) + R_a2 X2) + t_a.  Skip unless Y_z > 0.
 *   2. u = fx (Y_x / Y_z) + cx, v = fy (Y_y / Y_z) + cy, q = (floor(u + 0.5), floor(v + 0.5)).  Skip unless q lies in [0, W) x [0, H).
 *   3. d = D_v[q].  Skip if d is invalid.
 *   4. sdf = d - Y_z.  Skip unless sdf >= -trunc: a node farther than trunc behind the seen surface is occluded, not observed.
 *   5. S += min(1.0, sdf / trunc); W += 1.
 * Then sum = S, rounded once to the volume's dtype, and weight = W.  A comparison with a NaN fails.  No atomics: one thread owns a node
 * over the whole list, so the result depends only on the list order and two runs give the same bits.  A second integration continues
 * from the stored values.  The host keeps the number of views integrated since the volume was zeroed and refuses (PCS_ERR_ARG, before
 * the device is touched) a call that could take any weight past PCS_TSDF_MAX_WEIGHT = 65535.
 * Extraction, min_weight in [1, 65535].  A node is OBSERVED iff weight >= min_weight; its value is D = double(sum) / double(weight); it
 * is INSIDE iff it is observed and D < 0.  Cell (i, j, k) exists for i < nx - 1, j < ny - 1, k < nz - 1, with corners c = 0 .. 7 at node
 * (i + (c & 1), j + (c >> 1 & 1), k + (c >> 2 & 1)).  A cell is ACTIVE iff all eight corners are observed and they are neither all inside
 * nor all outside.
 *   Vertex of an active cell.  Walk the twelve cell edges (a, b) in the order (0,1) (0,2) (0,4) (1,3) (1,5) (2,3) (2,6) (3,7) (4,5) (4,6)
 *   (5,7) (6,7).  For an edge whose ends differ in INSIDE the crossing is p = the corner offset of a with the component along the edge's
 *   axis replaced by t = D_a / (D_a - D_b).  The crossings are added in edge order, per component, and each component is divided by
 *   their number: off.  The vertex is (o0 + s (i + off0), o1 + s (j + off1), o2 + s (k + off2)), rounded once to float32 or left as
 *   float64.  Vertices are numbered in the order of the cells' linear index (k (ny - 1) + j)(nx - 1) + i; every active cell gets a
 *   vertex, whether or not a quad uses it.
 *   Quads.  The grid edge from node n = (i, j, k) to its successor along axis A (0 = x, 1 = y, 2 = z): both ends must be observed and
 *   differ in INSIDE.  With (U, V) = (1, 2), (2, 0), (0, 1) for A = 0, 1, 2, the four cells around the edge are the cells at n offset by
 *   (dU, dV) = (-1, -1), (0, -1), (0, 0), (-1, 0) along axes U, V.  The edge emits one quad iff all four cells exist and are ACTIVE: the
 *   four vertex numbers in that order when n is INSIDE, in the reverse order otherwise, so that the quad's normal (v1 - v0) x (v3 - v0)
 *   points from inside to outside.  Quads are ordered by (A, node linear index).
 * Limits.  The ordered compaction is pcs_stereo_compact's, unchanged: the cell flags are nz - 1 "views" of (ny - 1)(nx - 1) pixels, the
 * quad flags 3 nz of ny nx.  Its limits (32767 views; one workgroup scans the block counts, however many) admit every grid up to
 * 1024^3, so PCS_TSDF_MAX_DIM is the only grid limit; vertex numbers are int32 (1023^3 < 2^31).  The volume is dense: 6 (float32 sum) or
 * 10 bytes per node, and the extraction's workspace 8 more per node.
 * Not done here: per-view weights, colour or intensity per vertex (row f19 below does it), marching cubes, a sparse or hashed volume, mesh smoothing or
 * simplification, distorted views (undistort first, pcs_imap_*).
 *   pcs_tsdf_create          a handle on `device` (no counterpart); it owns the view table, the volume and the extraction's workspace
 *   pcs_tsdf_destroy         frees the handle (no counterpart)
 *   pcs_tsdf_set_views       the arguments and checks of pcs_fuse_set_views.  The volume is kept.
 *   pcs_tsdf_set_grid        origin HOST (3), finite; voxel finite and > 0; nx, ny, nz in [1, 1024]; sum_dtype PCS_F32 or PCS_F64.
 *                            Allocates the volume and zeroes it.
 *   pcs_tsdf_reset           zeroes the volume and the count of integrated views
 *   pcs_tsdf_integrate       d_depth (n_views, height, width) of depth_dtype, the maps of ALL views of the table; views HOST (n_list)
 *                            int32 indices into the table, copied, or NULL: all views in order (n_list is then ignored).  An empty
 *                            list leaves the volume as it is.  One launch.
 *   pcs_tsdf_volume_ptrs     the device pointers of sum (nz, ny, nx) and weight, for tests and callers (either may be NULL)
 *   pcs_tsdf_extract_count   classifies the cells, numbers the vertices (a dense int32 cell -> vertex map, the hand-over to the quads),
 *                            flags the quads and scans both; returns the two counts to the host (blocking)
 *   pcs_tsdf_extract_write   fills d_vertices (n_vertices, 3) of vertex_dtype and d_quads (n_quads, 4) int32, buffers of exactly the
 *                            counted sizes (NULL allowed for a count of 0).  PCS_ERR_ARG when no count preceded it or the volume
 *                            changed since the count (an integration, a reset, a new grid).
 *   pcs_tsdf_last_kernel_ms  device time of the last integration, of the last count (classification, numbering, quad flags, scans) and
 *                            of the last write; any pointer may be NULL.  PCS_ERR_STATE when the part asked for has not run.
 * Every argument is checked on the host before the device is touched (PCS_ERR_ARG; pcs_last_error names the argument); the handle is
 * looked at last, and with it the view indices and the weight limit.  All buffers are DEVICE buffers of the caller unless marked HOST;
 * a run is queued on `stream` (NULL = the handle's).
 */
typedef struct pcs_tsdf_volume pcs_tsdf_volume;
enum { PCS_TSDF_MAX_DIM = 1024, PCS_TSDF_MAX_WEIGHT = 65535 };
int pcs_tsdf_create(pcs_tsdf_volume **out, int device);
int pcs_tsdf_destroy(pcs_tsdf_volume *p);
int pcs_tsdf_set_views(pcs_tsdf_volume *p, int64_t n_views, int width, int height, const double *K, const double *P);
int pcs_tsdf_set_grid(pcs_tsdf_volume *p, const double *origin, double voxel, int nx, int ny, int nz, int sum_dtype);
int pcs_tsdf_reset(pcs_tsdf_volume *p);
int pcs_tsdf_integrate(pcs_tsdf_volume *p, const void *d_depth, int depth_dtype, const int32_t *views, int64_t n_list, double trunc, void *stream);
int pcs_tsdf_volume_ptrs(pcs_tsdf_volume *p, void **d_sum, uint16_t **d_weight);
int pcs_tsdf_extract_count(pcs_tsdf_volume *p, int min_weight, int64_t *n_vertices, int64_t *n_quads, void *stream);
int pcs_tsdf_extract_write(pcs_tsdf_volume *p, void *d_vertices, int vertex_dtype, int32_t *d_quads, void *stream);
int pcs_tsdf_last_kernel_ms(pcs_tsdf_volume *p, float *integrate_ms, float *count_ms, float *write_ms);

/* ------------------------------------------------------------------------------------------------
 * Ray-cast of the TSDF volume: depth and normal maps of any view (csrc/ba_tsdf_raycast.hpp).  Since pcs_version() 128.
 * Replaces: nothing the reference computes.  It is KinectFusion's surface prediction on the volume above: the model's depth in a view,
 *           to hold against the measured depth map of that view, to fill its holes, to say which view sees a point, or to look at the
 *           scene from a pose no camera had.  The rule below is the library's own; tests/raycast_reference.py states it in NumPy.
 * The arithmetic is that of the block above: FP64, plain IEEE operations in the order written, no contraction, sums of three products
 * taken left to right, and a comparison with a NaN fails.  The volume, OBSERVED (weight >= min_weight) and D = double(sum) /
 * double(weight) are exactly those of the extraction.  n_a stands for (nx, ny, nz) and h_a = n_a - 1.
 * Render views.  They are independent of the integration's: distortion-free pinholes K = [fx, cx, fy, cy] with [R | t] world -> view,
 * and the call gives their width and height.  The host builds one table row per view: K, the nine entries of R, and the centre
 * C_a = -((R_0a t_0 + R_1a t_1) + R_2a t_2).
 * Ray of pixel (x, y).  r = ((x - cx) / fx, (y - cy) / fy, 1) and w_a = (R_0a r_0 + R_1a r_1) + R_2a r_2.  The world point at z-depth z
 * is C + z w: the parameter is the z-depth, as in every depth map of the library.  In grid units gc_a = (C_a - o_a) / s, gw_a = w_a / s.
 * Clip.  For each axis a: if gw_a == 0 the ray misses unless 0 <= gc_a <= h_a, and the axis bounds nothing; otherwise t0 = (0 - gc_a) /
 * gw_a, t1 = (h_a - gc_a) / gw_a and the axis contributes lo = min(t0, t1), hi = max(t0, t1).  z0 = max(z_near, the lo's), z1 =
 * min(z_far, the hi's).  The ray misses the box (status 3) unless every n_a >= 2 and z0 <= z1.
 * March.  dz = step / sqrt((w_0^2 + w_1^2) + w_2^2): samples are `step` apart in space.  q = (z1 - z0) / dz and N = floor(q).  The ray
 * also counts as missed (status 3) unless q <= 113513 (64 sqrt(3) 1024 + 1, rounded up), which holds for every R that is a rotation:
 * the loop is bounded for any finite table.  Sample n = 0 .. N sits at z_n = z0 + n dz, a product and never an accumulated sum, so that a
 * sample's position does not depend on which samples before it were evaluated.
 * Sample T(g) at g_a = gc_a + z gw_a.  Cell c_a = min(max(floor(g_a), 0), n_a - 2); fraction f_a = min(max(g_a - c_a, 0), 1).  The sample
 * is VALID iff the eight corners of cell c are OBSERVED.  Its value is the trilinear blend of the corners' D, each step in the form
 * (1 - f) A + f B, along x, then y, then z.  The two-product form is deliberate: with f in [0, 1] and all corners > 0 the result is > 0
 * exactly (short of underflow), and the skipping below rests on that.
 * Hit.  The first n >= 1 at which samples n - 1 and n are both VALID with T_{n-1} > 0 and T_n <= 0.  The depth is z = z_{n-1} + dz
 * (T_{n-1} / (T_{n-1} - T_n)).  A crossing from inside to outside, or one next to an invalid sample, is not a hit and the march goes on.
 * If no n qualifies the status is 2.
 * Normal at the hit point g = gc + z gw.  G_a = T(g + e_a) - T(g - e_a), central differences one node apart, taken in the order +x, -x,
 * +y, -y, +z, -z.  Each of the six samples needs 0 <= its coordinate <= h_b on every axis b and must be VALID.  n = G / sqrt((G_0^2 +
 * G_1^2) + G_2^2), in the world frame, pointing from inside to outside, stored as float32.  If a sample fails or |G| is not > 0 the
 * normal is NaN and the status 1; the depth is kept.
 * Outputs.  Depth (float32 or float64, the float64 value rounded once) is NaN where there is no hit: an invalid depth by the library's
 * own convention, so the map feeds pcs_fuse_run and pcs_tsdf_integrate unchanged.  Status is a uint8: PCS_TSDF_RAY_HIT 0,
 * PCS_TSDF_RAY_NO_NORMAL 1 (hit, no normal), PCS_TSDF_RAY_NO_CROSSING 2, PCS_TSDF_RAY_MISSED 3 (the box or the z-range).
 * Skipping empty space.  A mask pass runs before the cast, once per call because it depends on min_weight: it flags every brick of 8^3
 * cells one of whose corner nodes has weight >= min_weight and sum <= 0.  A sample whose cell lies in an unflagged brick is invalid or
 * > 0, can never be the second sample of a hit and is not evaluated; it can be the first, so on reaching a sample in a flagged brick
 * whose predecessor was skipped, the predecessor is evaluated for real.  flags bit 0, PCS_TSDF_RAYCAST_NO_SKIP, casts without the mask:
 * every output has the same bits either way.
 * Limits, checked on the host before the device is touched (PCS_ERR_ARG; pcs_last_error names the argument): views and sides as for
 * pcs_fuse_set_views; min_weight in [1, 65535]; step finite with voxel / 64 <= step, so that N <= 64 sqrt(3) 1024 + 1 and the kernel has
 * no open-ended loop; 0 <= z_near < z_far, where z_far may be +inf; a grid must be set.  The handle is looked at last.
 *   pcs_tsdf_raycast                 K (n_views, 4) and P (n_views, 12) HOST, copied.  d_depth (n_views, height, width) of depth_dtype;
 *                                    d_normal (n_views, height, width, 3) float32 or NULL: the six normal samples are then not taken
 *                                    and status 1 is not produced; d_status (n_views, height, width) or NULL.  The call reads the
 *                                    volume only: a preceding pcs_tsdf_extract_count stays valid for pcs_tsdf_extract_write, and the
 *                                    integration's view table is kept.  Two launches (mask, cast), one with PCS_TSDF_RAYCAST_NO_SKIP.
 *                                    The host waits for the handle's queued runs before it replaces the table of the render views.
 *   pcs_tsdf_raycast_last_kernel_ms  device time of the last cast's mask pass and of its cast kernel; either pointer may be NULL.
 *                                    PCS_ERR_STATE when the part asked for did not run.
 *   pcs_tsdf_raycast_count_samples   for measurements: the last pcs_tsdf_raycast over again in a separate launch (its views, settings
 *                                    and mask; none of its outputs is touched) that writes to d_samples (n_views, height, width) uint32
 *                                    the number of samples each pixel's march and normal evaluated.  The cast itself counts nothing.
 *                                    PCS_ERR_STATE when no cast ran on the volume as it stands.
 * Not done here: colour or intensity per pixel (row f19 below does it), distorted render views, a hierarchy deeper than one brick level or a stride over whole
 * bricks, a step that adapts to the distance value (it would tie a sample's position to the samples before it).
 */
enum { PCS_TSDF_RAY_HIT = 0, PCS_TSDF_RAY_NO_NORMAL = 1, PCS_TSDF_RAY_NO_CROSSING = 2, PCS_TSDF_RAY_MISSED = 3, PCS_TSDF_RAYCAST_NO_SKIP = 1 };
int pcs_tsdf_raycast(pcs_tsdf_volume *p, int64_t n_views, int width, int height, const double *K, const double *P, int min_weight, double step, double z_near,
                     double z_far, void *d_depth, int depth_dtype, float *d_normal, uint8_t *d_status, int flags, void *stream);
int pcs_tsdf_raycast_last_kernel_ms(pcs_tsdf_volume *p, float *mask_ms, float *cast_ms);
int pcs_tsdf_raycast_count_samples(pcs_tsdf_volume *p, uint32_t *d_samples, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Colour of surface points from the images (row f19): a colour per point from the source views that see it (SURVEY 8 row f19;
 * csrc/ba_tsdf_colour.hpp).  Since pcs_version() 129.
 * Replaces: nothing the reference computes; it draws what it reconstructs as coloured pyvista meshes.  This is the stage that brings the
 *           images the pipeline started from back onto the mesh of pcs_tsdf_extract_* and into the views of pcs_tsdf_raycast.  The rule
 *           below is the library's own; tests/colour_reference.py states it in NumPy.
 * The arithmetic is that of the two blocks above: FP64, plain IEEE operations in the order written, no contraction, sums of three
 * products taken left to right, and a comparison with a NaN fails.
 * Inputs.  Points X (N, 3), float32 or float64.  Optional unit normals n (N, 3) float32 in the world frame, pointing outward as the
 * ray-cast stores them.  A table of source views: K = [fx, cx, fy, cy] and [R | t] world -> view, distortion-free, all of one width x
 * height with both sides >= 2.  Source images (n_views, height, pitch BYTES), interleaved channels 1, 3 or 4, PCS_IMAP_U8 or
 * PCS_IMAP_F32.  Optional visibility depth maps (n_views, height, width), float32 or float64: normally the model's own depth from
 * pcs_tsdf_raycast into the source views; measured depth maps are allowed.
 * Per point and view, the views in list order:
 *   Y = R X + t, Y_a = ((R_a0 X_0 + R_a1 X_1) + R_a2 X_2) + t_a.  Rejected unless Y_2 > 0.
 *   u = fx (Y_0 / Y_2) + cx, w = fy (Y_1 / Y_2) + cy.  Rejected unless 0 <= u <= width - 1 and 0 <= w <= height - 1: every bilinear tap
 *   lies inside the image and no border colour enters a blend.
 *   Visibility, if maps are given: d at the nearest pixel (floor(u + 0.5), floor(w + 0.5)).  Rejected unless d is finite, d > 0 and
 *   Y_2 <= d + occlusion_tol (the sum first).  occlusion_tol is in world units.
 *   Angle, if normals are given: e_a = C_a - X_a with C the centre of the ray-cast's table, C_a = -((R_0a t_0 + R_1a t_1) + R_2a t_2);
 *   c = ((n_0 e_0 + n_1 e_1) + n_2 e_2) / sqrt((e_0^2 + e_1^2) + e_2^2).  Rejected unless c > cos_min; a NaN normal rejects every view.
 *   Without normals c = 1.
 *   Sample: cell x0 = min(floor(u), width - 2), fraction f = u - x0, and the same in y.  Each step of the blend has the form
 *   (1 - f) A + f B, along x for the upper and the lower row and then along y, per channel, in FP64 from the stored values.
 * Combination over the contributing views, in list order.  Wt = Wt + c from 0 in both modes.
 *   PCS_COLOUR_BLEND  S_k = S_k + c I_k from 0; colour_k = S_k / Wt.
 *   PCS_COLOUR_BEST   the sample of the view with the largest c; a tie goes to the lower list position.
 * Outputs.  colour (N, channels) PCS_IMAP_U8 or PCS_IMAP_F32: the FP64 value rounded once, the uint8 half-to-even and saturated as in
 * pcs_imap_remap (a NaN gives 0).  weight (N) float32 = Wt; count (N) uint16, the number of contributing views; best (N) int32, the list
 * position of the largest c (the lower on a tie) or -1.  A point without a contributing view gets fill[k] (HOST doubles, NULL means 0,
 * rounded like a colour), weight 0, count 0, best -1.  Any output pointer but colour may be NULL.
 * Limits, checked on the host before the device is touched (PCS_ERR_ARG; pcs_last_error names the argument): views as for
 * pcs_fuse_set_views with both sides >= 2; pitch a multiple of the element size and at least a row; occlusion_tol finite and >= 0 when
 * maps are given; cos_min in [0, 1); fill not infinite; min_weight in [1, 65535].  The handle is looked at last.
 *   pcs_tsdf_point_normals          the normal rule of the ray-cast at n arbitrary points (mesh vertices get normals): g = (X - o) / s,
 *                                   the six samples T(g +- e_a) through the cast's own sample function, each in the box and VALID, else
 *                                   the normal is three NaNs and the status 1 (0 otherwise).  A NaN point or one outside the box gives
 *                                   NaN.  d_normals (n, 3) float32; d_status (n) uint8 or NULL.  Needs a grid; reads the volume only.
 *   pcs_tsdf_colour_points          the rule on caller-supplied points.  K, P and fill HOST, copied; d_points, d_normals (or NULL),
 *                                   d_images, d_visibility (or NULL) and every output DEVICE.  It needs no grid.  n = 0 does nothing.
 *   pcs_tsdf_colour_views           the same rule with the pixels of n_render render views (K_render, P_render HOST; r_width x r_height)
 *                                   as the points: pixel (x, y) with z-depth z = d_depth (float32 or float64) is C + z w by the
 *                                   ray-cast's formulas, X_a = C_a + z w_a.  A depth that is not finite or not > 0 gives the fill.
 *                                   d_normal (n_render, r_height, r_width, 3) float32 or NULL: the outputs of pcs_tsdf_raycast.
 *                                   Outputs in image order (n_render, r_height, r_width, ...).
 *   pcs_tsdf_colour_last_kernel_ms  device time of the last pcs_tsdf_point_normals and of the last colour kernel; either pointer may be
 *                                   NULL.  PCS_ERR_STATE when the part asked for did not run.
 * The colour calls leave the volume, the integration's view table, a preceding pcs_tsdf_extract_count and the last cast as they are.
 * One launch each; the loop over the views runs inside the thread in list order, so two runs give identical bits.
 * Not done here: texture atlases and UV maps, distorted source views (undistort first: pcs_imap_remap), exposure or white-balance
 * compensation between views, colour stored in the volume during integration, seam levelling.
 */
enum { PCS_COLOUR_BLEND = 0, PCS_COLOUR_BEST = 1 };
int pcs_tsdf_point_normals(pcs_tsdf_volume *p, int64_t n, const void *d_points, int point_dtype, int min_weight, float *d_normals, uint8_t *d_status, void *stream);
int pcs_tsdf_colour_points(pcs_tsdf_volume *p, int64_t n, const void *d_points, int point_dtype, const float *d_normals, int64_t n_views, int width, int height,
                           const double *K, const double *P, const void *d_images, int64_t pitch, int channels, int image_dtype, const void *d_visibility,
                           int visibility_dtype, double occlusion_tol, double cos_min, int mode, const double *fill, void *d_colour, int colour_dtype, float *d_weight,
                           uint16_t *d_count, int32_t *d_best, void *stream);
int pcs_tsdf_colour_views(pcs_tsdf_volume *p, int64_t n_render, int r_width, int r_height, const double *K_render, const double *P_render, const void *d_depth,
                          int depth_dtype, const float *d_normal, int64_t n_views, int width, int height, const double *K, const double *P, const void *d_images,
                          int64_t pitch, int channels, int image_dtype, const void *d_visibility, int visibility_dtype, double occlusion_tol, double cos_min, int mode,
                          const double *fill, void *d_colour, int colour_dtype, float *d_weight, uint16_t *d_count, int32_t *d_best, void *stream);
int pcs_tsdf_colour_last_kernel_ms(pcs_tsdf_volume *p, float *normals_ms, float *colour_ms);

/* ------------------------------------------------------------------------------------------------
 * The target pose of every image in a calibrated rig (csrc/ba_rigpose.hpp).  Since pcs_version() 110.
 * Replaces: find_target_pose_at_timestep and find_target_poses (optimisation/find_target.py:9-82), which fix every camera's "ext", "int"
 *           and "dst" and run the whole bundle adjustment for the target poses that are left.  With the cameras fixed the problem is one
 *           independent 6-parameter least-squares problem per image over the detections of all cameras that see it; every image is
 *           solved by its own group of lanes with its own damping, and a converged image is frozen while its neighbours continue.
 * Unknown per image: T = (R, t), target -> world, as [rotvec, t].  Residual of a detection (camera c, key k): uv - project_c(E_c (R X_k + t))
 * in the measured pixels, full Brown-Conrady model; update R <- exp([d omega]x) R, t <- t + d t.  Damping, accept rule, stops and status
 * codes are those of pcs_pnp_run; a point counts as behind when it is behind ITS camera.  No floating-point atomics, every sum in a fixed
 * order: for a given group width two runs give the same bits; the two widths differ in rounding only.
 *   pcs_rigpose_create            n_cams cameras, a template of n_keys points (no counterpart: a handle)
 *   pcs_rigpose_destroy           frees the handle (no counterpart)
 *   pcs_rigpose_set_cameras       intr (n_cams, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2], held fixed (find_target.py:9-82 puts "int" and
 *                                 "dst" of every camera into fixed_params)
 *   pcs_rigpose_set_extrinsics    ext (n_cams, 12) world -> camera, rows [R | t] of a 3 x 4 transform, held fixed (the "ext" of
 *                                 find_target.py:9-82); the convention of pcs_rig_set_extrinsics
 *   pcs_rigpose_set_template      points (n_keys, 3): target.point_data flattened (find_target.py:9-82 hands the target to the handler)
 *   pcs_rigpose_set_observations  host arrays, copied: key (n_obs) int32, cam (n_obs) int32, uv (n_obs, 2), sorted by (image, camera,
 *                                 key); group j (one image) owns rows [start_inds[j], start_inds[j+1]).  Inside a group cam must not
 *                                 decrease -> PCS_ERR_ARG; cameras and keys are range-checked -> PCS_ERR_RANGE; the first bad group
 *                                 decides the refusal.  Forgets the start poses.  (find_target.py:9-82 selects the detections of the
 *                                 time step the same way)
 *   pcs_rigpose_set_start         poses (n_groups, 6) = [rotvec, t] of the start, after the observations (find_target.py:9-82 starts
 *                                 from calc_initial_params)
 *   pcs_rigpose_run               queue the kernel on `stream` (NULL = the handle's stream).  group_lanes: 16 or 64 lanes per image, 0
 *                                 = 64 when the mean number of observations per image is at least 256, else 16.  A group with fewer
 *                                 than min_points observations, a non-finite start or a point behind its camera at the start is not
 *                                 estimated: NaN pose, status 0.  Outputs (device buffers of the caller, or NULL = handle-owned):
 *                                 d_pose (n_groups, 6); d_rms (n_groups, 2) RMS reprojection error at the returned pose and at the
 *                                 start, pixels; d_info (n_groups, 4) int32 {trials used, status PCS_RIGPOSE_*, observations, cameras
 *                                 that contributed}; d_hess (n_groups, 21) the packed upper triangle of J'J at the returned pose by
 *                                 rows (00 01 .. 05 11 .. 55; NaN when not estimated); with flags PCS_RIGPOSE_RESIDUALS, d_resid
 *                                 (n_obs, 2) residuals at the returned pose in observation order.  PCS_ERR_ARG: NULL handle,
 *                                 max_iter < 0, a negative or non-finite tolerance, min_points < 1, another group_lanes, unknown flags.
 *                                 (replaces the optimiser call of find_target.py:9-82)
 *   pcs_rigpose_results           copy handle-owned outputs of the last run to the host (any pointer may be NULL; blocking) (the poses
 *                                 find_target.py:9-82 reads back from the optimised parameter vector)
 *   pcs_rigpose_last_kernel_ms    device time of the last run: ordering of the images and the LM kernel.  PCS_ERR_STATE when the last
 *                                 run had no images and so queued nothing (no counterpart).
 */
typedef struct pcs_rig_localiser pcs_rig_localiser;
#define PCS_RIGPOSE_RESIDUALS 1
enum {
    PCS_RIGPOSE_NOT_ESTIMATED = 0,   /* too few observations, a non-finite start or a point behind its camera at the start: the pose is NaN */
    PCS_RIGPOSE_CONVERGED = 1,       /* ftol, xtol or gtol */
    PCS_RIGPOSE_MAX_ITER = 2,        /* max_iter trials used */
    PCS_RIGPOSE_NO_DECREASE = 3      /* the damping grew past 1e10 without a lower cost, or the damped system lost definiteness */
};
enum { PCS_RIGPOSE_OUT_POSE = 1, PCS_RIGPOSE_OUT_RMS = 2, PCS_RIGPOSE_OUT_INFO = 4, PCS_RIGPOSE_OUT_HESSIAN = 8, PCS_RIGPOSE_OUT_RESIDUALS = 16 };
int pcs_rigpose_create(pcs_rig_localiser **out, int device, int64_t n_cams, int64_t n_keys);
int pcs_rigpose_destroy(pcs_rig_localiser *p);
int pcs_rigpose_set_cameras(pcs_rig_localiser *p, const double *intr);
int pcs_rigpose_set_extrinsics(pcs_rig_localiser *p, const double *ext);
int pcs_rigpose_set_template(pcs_rig_localiser *p, const double *points);
int pcs_rigpose_set_observations(pcs_rig_localiser *p, int64_t n_obs, const int32_t *key, const int32_t *cam, const double *uv, int64_t n_groups,
                                 const int64_t *start_inds);
int pcs_rigpose_set_start(pcs_rig_localiser *p, const double *poses);
int pcs_rigpose_run(pcs_rig_localiser *p, int max_iter, double ftol, double xtol, double gtol, int min_points, int group_lanes, int flags,
                    double *d_pose, double *d_rms, int32_t *d_info, double *d_hess, double *d_resid, void *stream);
int pcs_rigpose_results(pcs_rig_localiser *p, double *pose, double *rms, int32_t *info, double *hess, double *resid);
int pcs_rigpose_last_kernel_ms(pcs_rig_localiser *p, float *kernel_ms);
/* Robust loss of the per-image solve (since pcs_version() 113; the reference's commented `loss = "cauchy"` on the least_squares call
 * find_target.py:9-82 goes through).  The kinds, the formulas and the validation are those of pcs_set_loss, applied to each scalar
 * residual (u and v separately): H = sum s^2 J'J, g = sum J' rho1 f.  The cost the accept rule, ftol and the test of the start look at
 * is sum rho0; the depth test, the damping, xtol, gtol (on the robust g) and the statuses keep their rules.  d_rms stays the plain pixel
 * RMS and d_resid the raw residuals; d_hess holds the robust H.  The setting belongs to the handle and survives new cameras and
 * observations; PCS_LOSS_LINEAR, the default, launches the kernel of a handle on which no loss was ever set.
 *   pcs_rigpose_set_loss  mirrors pcs_set_loss.  PCS_ERR_ARG (the previous setting stays in force): NULL handle, a kind outside
 *                         PCS_LOSS_*, an f_scale that is not finite and > 0.
 *   pcs_rigpose_get_loss  mirrors pcs_get_loss (either pointer may be NULL).
 *   pcs_rigpose_costs     mirrors pcs_rigpose_results for one more output: cost (n_groups, 2) = 0.5 sum rho0 (scipy's cost) at the
 *                         returned pose and at the start, NaN when not estimated, always handle-owned (blocking).  After a LINEAR run
 *                         the costs are derived in this call, 0.5 n rms^2 from the RMS that run wrote (read on the device where it
 *                         wrote it: the handle's output or the caller's d_rms, which must still hold it); the run itself queues
 *                         what it queued before a loss existed.  PCS_ERR_ARG: NULL handle or array; PCS_ERR_STATE: no run on the
 *                         current inputs. */
int pcs_rigpose_set_loss(pcs_rig_localiser *p, int kind, double f_scale);
int pcs_rigpose_get_loss(pcs_rig_localiser *p, int *kind, double *f_scale);
int pcs_rigpose_costs(pcs_rig_localiser *p, double *cost);

/* ------------------------------------------------------------------------------------------------
 * Camera intrinsics from planar target views (csrc/ba_intrinsics.hpp).  Since pcs_version() 106.
 * Replaces: AbstractTarget.initial_calibration (calibration_targets/abstract_target.py:263-343: per camera every (image, board) group
 *           with more than 12 detections goes to cv2.calibrateCamera), the rough intrinsics calc_initial_params starts from
 *           (optimisation/template_handler.py:321-329 reads them from the camera set).  The closed form of that call: Zhang's method
 *           with zero skew ("full") and OpenCV's initCameraMatrix2D, principal point at the image centre ("focal"); no distortion.
 * A group is the set of detections of one (camera, image, board) triple.  Per group a homography pixels <- plane frame (h33 = 1, 8 x 8
 * normal equations, Hartley-normalised pixels; the plane frame is the PnP start's: centroid c, in-plane axes e1, e2 of the template
 * points' scatter, metres); per camera the constraints h1' B h2 = 0, h1' B h1 = h2' B h2 of its groups on B = K^-T K^-1.
 *   pcs_intr_create            n_cams cameras, a template of n_keys points
 *   pcs_intr_set_template      points (n_keys, 3): target.point_data flattened (abstract_target.py:307 gathers the same per board from point_local)
 *   pcs_intr_set_observations  host arrays, copied: key (n_obs) int32, uv (n_obs, 2), sorted by group; group j owns rows
 *                              [start_inds[j], start_inds[j+1]) and belongs to camera group_cam[j]; the groups are sorted by camera;
 *                              keys and cameras are range-checked -> PCS_ERR_RANGE (abstract_target.py:297-310 gathers the same)
 *   pcs_intr_run               queue the two kernels on `stream` (NULL = the handle's stream).  model: PCS_INTR_MODEL_*; AUTO is FOCAL
 *                              when res is given (what OpenCV does) and FULL otherwise.  min_points >= 4 (the reference: 13, "more
 *                              than 12", abstract_target.py:306).  res: host (n_cams, 2) = (h, w) per camera, or NULL: the normalising
 *                              centre ((w - 1) / 2, (h - 1) / 2) and scale (w + h) / 2; without it the count-weighted mean of the
 *                              groups' pixel centroids and spreads.  A group with too few observations, a non-planar template, a
 *                              non-finite measurement or a failed fit contributes nothing (its status says why).  The full model falls
 *                              back to the focal one (status PCS_INTR_FOCAL_FALLBACK) when B is not definite, the camera has fewer
 *                              than two used groups, V'V has more than one vanishing eigenvalue, or the result is not finite.
 *                              Outputs (device buffers of the caller, or NULL = handle-owned): d_intr (n_cams, 9) =
 *                              [fx, cx, fy, cy, 0, 0, 0, 0, 0] (NaN when not estimated); d_cam_info (n_cams, 2) int32 {status
 *                              PCS_INTR_*, groups used}; d_eig_ratio (n_cams) smallest / second smallest eigenvalue of V'V (near 1:
 *                              the views do not constrain the model); d_homographies (n_groups, 9) row-major; d_frames (n_groups, 9)
 *                              = [c, e1, e2]; d_group_info (n_groups, 2) int32 {status PCS_INTR_GROUP_*, observations};
 *                              d_pixel_stats (n_groups, 3) = pixel centroid and mean distance from it.
 *                              PCS_ERR_ARG: NULL handle, unknown model, min_points < 4, a non-finite or non-positive res.
 *   pcs_intr_results           copy handle-owned outputs of the last run to the host (any pointer may be NULL; blocking)
 *                              (replaces the camera matrix cv2.calibrateCamera returns, abstract_target.py:313-333)
 *   pcs_intr_last_kernel_ms    device time of the last run: both kernels, and the consensus stage when it is on.
 *
 * Consensus sampling (csrc/ba_intr_consensus.hpp; since pcs_version() 117), opt-in: what cv2.findHomography(..., RANSAC) is to the plain
 * fit, at the same place in the pipeline (abstract_target.py:263-343).  One detection with a wrong id bends the homography of its group,
 * and a few bent homographies lose the camera.  With the stage on, n_hypotheses samples of sample_size detections per group are fitted
 * by the same homography kernel, every hypothesis is scored on all detections of the group by sum min(e^2, inlier_px^2) of the transfer
 * error e = uv - H q (tau^2 for a non-finite term and for a point beyond the plane's horizon), and the homography and camera kernels
 * then run on the detections within inlier_px of the best hypothesis.  The sampler is the PnP stage's: counter-based, keyed by (seed,
 * camera, observations of the group, hypothesis); the hypothesis count is fixed, so two runs agree bit for bit, and a table without
 * outliers gives the bits of the plain run.  A homography knows no lens distortion: inlier_px has to cover what the lens bends.
 *   pcs_intr_set_consensus     n_hypotheses = 0 (the default) turns the stage off: pcs_intr_run then queues what it always queued and
 *                              allocates nothing more.  Otherwise cv2.findHomography's maxIters, the sample (4 <= sample_size <= 16),
 *                              ransacReprojThreshold and the seed of the generator.  PCS_ERR_ARG: NULL handle, a negative count,
 *                              n_hypotheses > 4096, sample_size outside [4, 16], inlier_px not finite or <= 0; a refused call keeps
 *                              the previous setting.
 *   pcs_intr_get_consensus     the setting in force (any pointer may be NULL; cv2.findHomography's arguments, which it does not keep)
 *   pcs_intr_consensus_results copy what the stage of the last run found to the host (cv2.findHomography's `mask`; blocking, any
 *                              pointer may be NULL): inlier (n_obs) one flag per observation; cinfo (n_groups, 4) int32 {inliers, winning
 *                              hypothesis or -1, hypotheses with a finite homography, consensus used}; score (n_groups) the winner's
 *                              sum min(e^2, inlier_px^2) (+inf: no finite hypothesis, NaN: consensus not used).  A group with fewer
 *                              observations than max(sample_size, min_points) takes the plain path (all flagged, consensus used = 0);
 *                              so does a group without a finite hypothesis (all flagged, consensus used = 1), whose status then names
 *                              the reason as the plain run does (NOT_PLANAR, NOT_FINITE); a group whose winner has fewer than
 *                              min_points inliers is PCS_INTR_GROUP_TOO_FEW; a NaN measurement is never an inlier.  With the stage on,
 *                              d_group_info keeps the group's observation count, and the camera's normalising centre weights the
 *                              groups by their inlier counts: every output is the plain run's on the inlier rows.
 *                              PCS_ERR_STATE when the last run had no consensus stage.
 */
typedef struct pcs_intrinsics_estimator pcs_intrinsics_estimator;
enum { PCS_INTR_MODEL_AUTO = 0, PCS_INTR_MODEL_FULL = 1, PCS_INTR_MODEL_FOCAL = 2 };
enum {
    PCS_INTR_NOT_ESTIMATED = 0,    /* no usable group, or the focal system is singular or gave a non-positive 1 / f^2: the row is NaN */
    PCS_INTR_FULL = 1,             /* fx, cx, fy, cy from B */
    PCS_INTR_FOCAL = 2,            /* the focal model was asked for: fx, fy, the principal point at the normalising centre */
    PCS_INTR_FOCAL_FALLBACK = 3    /* the full model was asked for and could not be used */
};
enum {
    PCS_INTR_GROUP_TOO_FEW = 0,     /* fewer than min_points observations */
    PCS_INTR_GROUP_USED = 1,
    PCS_INTR_GROUP_NOT_PLANAR = 2,  /* lambda_min >= 1e-3 lambda_mid of the template points' scatter (the PnP start's rule) */
    PCS_INTR_GROUP_NOT_FINITE = 3,  /* a non-finite measurement, or all measurements in one pixel */
    PCS_INTR_GROUP_FIT_FAILED = 4   /* the homography's normal equations lost definiteness */
};
enum { PCS_INTR_OUT_INTR = 1, PCS_INTR_OUT_CAM_INFO = 2, PCS_INTR_OUT_EIG_RATIO = 4, PCS_INTR_OUT_HOMOGRAPHIES = 8, PCS_INTR_OUT_FRAMES = 16,
       PCS_INTR_OUT_GROUP_INFO = 32, PCS_INTR_OUT_PIXEL_STATS = 64 };
int pcs_intr_create(pcs_intrinsics_estimator **out, int device, int64_t n_cams, int64_t n_keys);
int pcs_intr_destroy(pcs_intrinsics_estimator *p);
int pcs_intr_set_template(pcs_intrinsics_estimator *p, const double *points);
int pcs_intr_set_observations(pcs_intrinsics_estimator *p, int64_t n_obs, const int32_t *key, const double *uv, int64_t n_groups, const int64_t *start_inds,
                              const int32_t *group_cam);
int pcs_intr_run(pcs_intrinsics_estimator *p, int model, int min_points, const double *res, double *d_intr, int32_t *d_cam_info, double *d_eig_ratio,
                 double *d_homographies, double *d_frames, int32_t *d_group_info, double *d_pixel_stats, void *stream);
int pcs_intr_results(pcs_intrinsics_estimator *p, double *intr, int32_t *cam_info, double *eig_ratio, double *homographies, double *frames,
                     int32_t *group_info, double *pixel_stats);
int pcs_intr_last_kernel_ms(pcs_intrinsics_estimator *p, float *kernel_ms);
int pcs_intr_set_consensus(pcs_intrinsics_estimator *p, int n_hypotheses, int sample_size, double inlier_px, uint64_t seed);
int pcs_intr_get_consensus(pcs_intrinsics_estimator *p, int *n_hypotheses, int *sample_size, double *inlier_px, uint64_t *seed);
int pcs_intr_consensus_results(pcs_intrinsics_estimator *p, uint8_t *inlier, int32_t *cinfo, double *score);

/* ------------------------------------------------------------------------------------------------
 * View-graph seeding of a rig (csrc/ba_riggraph.hpp).  Since pcs_version() 107.
 * Replaces: estimate_camera_relative_poses (optimisation/template_handler.py:468-601), which takes the target of one image that EVERY
 *           camera sees as the world and raises where there is none (template_handler.py:454-466), and scores the per-image candidates
 *           with one pass of the legacy cost per camera (template_handler.py:528-578).  Here the co-visibility graph only has to be
 *           connected.  M[c, i] is the view transform target -> camera c in image i (pcs_pnp_results; NaN where not estimated); a
 *           3 x 4 transform is 12 doubles, rows [R | t].
 *   pcs_rig_create            n_cams cameras (<= 46340), n_imgs images, a template of n_keys points (no counterpart: a handle)
 *   pcs_rig_destroy           frees the handle (no counterpart)
 *   pcs_rig_set_cameras       intr (n_cams, 9) = [fx, cx, fy, cy, k0, k1, p0, p1, k2] (template_handler.py:504-507: K and dists)
 *   pcs_rig_set_template      points (n_keys, 3): target.point_data flattened (template_handler.py:511).  frame (4 doubles, or NULL)
 *                             receives the centroid pbar and the RMS distance rho of the points from it.
 *   pcs_rig_set_observations  host arrays, copied: as pcs_pnp_set_observations, plus view_im (n_views) the image of every view; views
 *                             sorted by (camera, image); cameras, images and keys are range-checked -> PCS_ERR_RANGE
 *                             (template_handler.py:537-543 hands the same table to the cost)
 *   pcs_rig_set_view_poses    poses (n_cams, n_imgs, 6) = [rotvec, t] of M[c, i], NaN where there is none (the Mat_ac array of
 *                             template_handler.py:484-491)
 *   pcs_rig_run_edges         queue the edge consensus on `stream` (NULL = the handle's): per camera pair a < b (lexicographic order,
 *                             n_cams (n_cams - 1) / 2 pairs) the candidates T_i = M[a, i] inv(M[b, i]) of the n images both see, the
 *                             distance d(T_i, T_j)^2 = (rho^2 / 3)(6 - 2 tr(R_i' R_j)) + |(R_i - R_j) m_b + t_i - t_j|^2 with
 *                             m_b = mean_j M[b, j] pbar, and the medoid: the candidate of smallest S_i = sum_j d(T_i, T_j), ties to the
 *                             lowest image (replaces the single reference image of template_handler.py:493-497)
 *   pcs_rig_edges             copy the edge outputs to the host (any pointer may be NULL; blocking): info (pairs, 2) int32 {n, medoid
 *                             image or -1}; T (pairs, 12) camera b -> camera a (NaN for n = 0); stats (pairs, 3) = {sigma = S / (n - 1)
 *                             (0 for n = 1, NaN for n = 0), S of the medoid, S of the runner-up (+inf for n < 2)}
 *   pcs_rig_set_extrinsics    ext (n_cams, 12) world -> camera, composed by the caller along a tree through the pairs (the Mrt_ac of
 *                             template_handler.py:497)
 *   pcs_rig_run_scores        queue the scoring: W[c', i] = inv(E_c') M[c', i] for every camera and image (template_handler.py:499-502,
 *                             without the forward fill of :528-532) and, for every view (c, i) and every candidate camera c', the sum over
 *                             the view's detections of |project_c(E_c W[c', i] p_k) - uv| with the legacy cost's formulas
 *                             (compiled_helpers.py:518-549) -> partial[c', view]; errors[c', i] adds the views of image i in view order
 *                             (template_handler.py:535-560 for all cameras in one pass over the table).  NaN where W[c', i] is.
 *   pcs_rig_results           copy the scoring outputs to the host (any pointer may be NULL; blocking): W (n_cams, n_imgs, 12),
 *                             errors (n_cams, n_imgs), partial (n_cams, n_views) (the `errors` list of template_handler.py:518-560)
 *   pcs_rig_last_kernel_ms    device time of the last edge run (view matrices + edge kernel), of the last preparation (W and the
 *                             projections) and of the last scoring (score + per-image sums); any pointer may be NULL.  PCS_ERR_STATE
 *                             when the run asked for has not happened.
 *   PCS_ERR_STATE from a run whose inputs are not all set, and from a read-back without a run on the current inputs.
 */
typedef struct pcs_rig_graph pcs_rig_graph;
int pcs_rig_create(pcs_rig_graph **out, int device, int64_t n_cams, int64_t n_imgs, int64_t n_keys);
int pcs_rig_destroy(pcs_rig_graph *p);
int pcs_rig_set_cameras(pcs_rig_graph *p, const double *intr);
int pcs_rig_set_template(pcs_rig_graph *p, const double *points, double *frame);
int pcs_rig_set_observations(pcs_rig_graph *p, int64_t n_obs, const int32_t *key, const double *uv, int64_t n_views, const int64_t *start_inds,
                             const int32_t *view_cam, const int32_t *view_im);
int pcs_rig_set_view_poses(pcs_rig_graph *p, const double *poses);
int pcs_rig_run_edges(pcs_rig_graph *p, void *stream);
int pcs_rig_edges(pcs_rig_graph *p, int32_t *info, double *T, double *stats);
int pcs_rig_set_extrinsics(pcs_rig_graph *p, const double *ext);
int pcs_rig_run_scores(pcs_rig_graph *p, void *stream);
int pcs_rig_results(pcs_rig_graph *p, double *W, double *errors, double *partial);
int pcs_rig_last_kernel_ms(pcs_rig_graph *p, float *edges_ms, float *prepare_ms, float *scores_ms);

/* ------------------------------------------------------------------------------------------------
 * Per-group reprojection statistics of a residual vector on the device (csrc/ba_groupstats.hpp).  Since pcs_version() 108.
 * Replaces: what a user does after the solve, on the host, from a read-back residual: the mean of optimisation_handling.py:66-70
 *           (mean_reprojection_error), the per-image error and its MAD test (optimisation/template_handler.py:242-279 with
 *           utils/general_utils.py:108-133), and the per-view RMS that cv2.calibrateCameraExtended returns as perViewErrors.
 * Per detection e = sqrt(ru^2 + rv^2); a detection whose e is not finite is counted in n_nonfinite and takes no part in anything else.
 * Groupings (PCS_STATS_BY_*): camera (n_cams groups), image (n_imgs), key (n_keys), view = (camera, image) (n_cams * n_imgs, group
 * c * n_imgs + i) and PCS_STATS_OVERALL, one group over all rows.  A group may be empty.  Inside a group the rows are taken in ascending
 * table order, whatever the order of the table; sums go through fixed trees and there are no floating-point atomics: two runs give the
 * same bits.  Median and MAD (median of |e - median|) are exact: the middle order statistic, or (a + b) * 0.5 of the two middle ones.
 *   pcs_stats_create             n_cams, n_imgs, n_keys: the group counts (no counterpart: a handle)
 *   pcs_stats_destroy            frees the handle (no counterpart)
 *   pcs_stats_set_groups         host arrays cam, img, key (n) int32, the id columns of the detection table, in table order (the columns
 *                                template_handler.py:537-543 hands to the per-image cost); an id outside [0, count) -> PCS_ERR_RANGE.
 *                                Builds the group index on the device (a stable radix sort of the rows by group); it is kept until
 *                                the next call.  A refused table leaves the handle without groups.  Blocking.
 *   pcs_stats_set_groups_device  the same from device arrays; the range check runs on the device (PCS_ERR_RANGE names the lowest bad
 *                                row, and the handle then has no groups).  Blocking.
 *   pcs_stats_run                queue the kernels on `stream` (NULL = the handle's stream).  d_resid: 2 n doubles [u0, v0, u1, v1, ...]
 *                                on the device: pcs_device_buffers / pcs_genchain_device_buffers of a PCS_F64 engine, or the caller's
 *                                own (what optimisation_handling.py:66-70 reshapes to (-1, 2) on the host).  flags:
 *                                PCS_STATS_NO_ORDER_STATISTICS leaves median and mad NaN and skips the selection.  Outputs (device
 *                                buffers of the caller, or NULL = handle-owned), G = n_cams + n_imgs + n_keys + n_cams * n_imgs + 1
 *                                groups in the order camera, image, key, view, overall: d_errors (n) = e; d_counts (3, G) int32 =
 *                                count of finite rows, n_nonfinite, argmax (the table row of the largest finite e, the lowest row of
 *                                equal ones, -1 for a group without finite rows); d_values (7, G) = sum_e, sum_e2, sum_ru, sum_rv,
 *                                max_e, median, mad (max_e, median and mad are NaN for a group without finite rows).
 *                                PCS_ERR_STATE: no groups set.
 *   pcs_stats_results            copy one grouping's handle-owned outputs of the last run to the host (any pointer may be NULL;
 *                                blocking); every array has the grouping's number of groups.  sum_e / count is the mean error (the
 *                                overall one: optimisation_handling.py:66-70), sqrt(sum_e2 / count) the RMS (per view: OpenCV's
 *                                perViewErrors), sum_ru / count and sum_rv / count the bias; median and mad are what
 *                                utils/general_utils.py:108-133 computes on the host.  PCS_ERR_STATE: no run on the current groups,
 *                                or the run wrote the asked outputs to caller buffers.
 *   pcs_stats_errors             copy the handle-owned e (n) of the last run to the host (blocking) (the per-detection norm of
 *                                optimisation_handling.py:66-70)
 *   pcs_stats_last_kernel_ms     device time of the last index build, of the last error kernel and of the last statistics (gather +
 *                                statistics kernel); any pointer may be NULL.  PCS_ERR_STATE when the part asked for has not run.
 */
typedef struct pcs_residual_stats pcs_residual_stats;
enum { PCS_STATS_BY_CAMERA = 0, PCS_STATS_BY_IMAGE = 1, PCS_STATS_BY_KEY = 2, PCS_STATS_BY_VIEW = 3, PCS_STATS_OVERALL = 4 };
#define PCS_STATS_NO_ORDER_STATISTICS 1
enum { PCS_STATS_OUT_ERRORS = 1, PCS_STATS_OUT_COUNTS = 2, PCS_STATS_OUT_VALUES = 4 };
int pcs_stats_create(pcs_residual_stats **out, int device, int64_t n_cams, int64_t n_imgs, int64_t n_keys);
int pcs_stats_destroy(pcs_residual_stats *p);
int pcs_stats_set_groups(pcs_residual_stats *p, int64_t n, const int32_t *cam, const int32_t *img, const int32_t *key);
int pcs_stats_set_groups_device(pcs_residual_stats *p, int64_t n, const int32_t *d_cam, const int32_t *d_img, const int32_t *d_key);
int pcs_stats_run(pcs_residual_stats *p, const double *d_resid, int flags, double *d_errors, int32_t *d_counts, double *d_values, void *stream);
int pcs_stats_results(pcs_residual_stats *p, int grouping, int32_t *count, int32_t *n_nonfinite, int32_t *argmax, double *sum_e, double *sum_e2,
                      double *sum_ru, double *sum_rv, double *max_e, double *median, double *mad);
int pcs_stats_errors(pcs_residual_stats *p, double *errors);
int pcs_stats_last_kernel_ms(pcs_residual_stats *p, float *index_ms, float *error_ms, float *stats_ms);

/* Page-locked host memory for outputs: pcs_eval / pcs_eval_compact copy device -> host at PCIe rate
 * into such buffers (a pageable destination is several times slower).  Replaces nothing in the
 * reference (NumPy owns every array there, afb:561); SURVEY 8 f1 "zero-copy hand-off". */
int pcs_host_alloc(void **out, int64_t bytes);
int pcs_host_free(void *p);
/* Streaming probe of the device's achievable HBM rate with this engine's access shape (16 B per lane):
 * kind 0 fill, 1 non-temporal fill, 2 copy, 3 non-temporal copy, 4 non-temporal fill in the fused kernel's
 * shape (every wave writes whole 10 752-byte chunks), 5..8 the same with 21 KiB / 1 KiB / 64 KiB / 256 KiB chunks;
 * `bytes` per launch (per buffer).
 * Measurement aid for DESIGN.md / bench.py --membench; not on the evaluation path. */
int pcs_membench(int device, int kind, int64_t bytes, int iters, int blocks_per_cu, float *mean_ms);
/* Engine-owned device scratch for outputs (engine dtype); valid until the next set_detections. */
int pcs_device_buffers(pcs_engine *h, void **d_resid, void **d_jac);

#ifdef __cplusplus
}
#endif
#endif /* PCS_HIP_H */
