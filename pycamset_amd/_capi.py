"""ctypes binding of the C ABI in include/pcs_hip.h (libpcs_hip.so, built in-tree by
``__graft_entry__.build()`` / ``python -m pycamset_amd.build``).

There is no fallback: if the shared library is missing or no HIP device is visible the
product path raises (PcsError / OSError) — it never routes through NumPy or the CPU oracle.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint8, c_uint64, c_void_p
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libpcs_hip.so"

PCS_OK, PCS_ERR_ARG, PCS_ERR_HIP, PCS_ERR_STATE, PCS_ERR_NODEVICE, PCS_ERR_RANGE = 0, -1, -2, -3, -4, -5
CHAIN_IDS = {"template": 0, "self": 1, "free": 2}
CHAIN_P = {"template": 21, "self": 24, "free": 18}
DTYPE_IDS = {"f64": 0, "f32": 1, "mixed": 2}   # mixed: FP64 arithmetic, FP32 residual / Jacobian bytes
# robust losses of the normal equations (include/pcs_hip.h PCS_LOSS_*): scipy.optimize.least_squares's names
LOSS_IDS = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}

# every symbol include/pcs_hip.h declares: name -> (restype, argtypes)
_P = c_void_p
class LmBuffers(ctypes.Structure):
    """include/pcs_hip.h pcs_lm_buffers: the device buffers of one LM trial (pcs_lm_trial_build / pcs_lm_trial_finish)."""
    _fields_ = [("packed", c_void_p * 2), ("ps", c_void_p * 2)] + [
        (n, c_void_p) for n in ("flags", "fixed", "lam", "linvt", "u", "V", "S", "rhs", "dvec", "gm", "status", "xlead", "w", "spd_work", "delta", "ctrl", "stats",
                                "stats_host")] + [
        ("spd_algorithm", ctypes.c_int32), ("mode", ctypes.c_int32), ("free_idx", c_void_p), ("n_free", ctypes.c_int64), ("result_host", c_void_p),
        ("syrk_work", c_void_p), ("syrk_work_len", ctypes.c_int64)]


LM_FIXED_TRIAL_BUFFER, LM_VOTES = 1, 2   # include/pcs_hip.h PCS_LM_*
LM_STATS = 12                            # doubles in a trial's read-back (and in the control block)
COV_TRSM_IDENTITY = 1                    # include/pcs_hip.h PCS_COV_TRSM_IDENTITY
TRI_REFINE_RESIDUALS = 1                 # include/pcs_hip.h PCS_TRI_REFINE_RESIDUALS
# include/pcs_hip.h PCS_TRI_REFINE_*: per-point status of the triangulation refinement
TRI_NOT_REFINED, TRI_CONVERGED, TRI_MAX_ITER, TRI_NO_DECREASE = 0, 1, 2, 3
PNP_RESIDUALS = 1                        # include/pcs_hip.h PCS_PNP_RESIDUALS
# include/pcs_hip.h PCS_PNP_*: per-view status of the pose estimation
PNP_NOT_ESTIMATED, PNP_CONVERGED, PNP_MAX_ITER, PNP_NO_DECREASE = 0, 1, 2, 3
# include/pcs_hip.h PCS_TWOVIEW_*: per-pair status of the two-view consensus
TWOVIEW_OK, TWOVIEW_TOO_FEW, TWOVIEW_DEGENERATE, TWOVIEW_NO_CHEIRALITY = 0, 1, 2, 3
# include/pcs_hip.h PCS_TWOVIEW_EIGHT_POINT / PCS_TWOVIEW_FIVE_POINT: the hypothesis solver of pcs_twoview_set_solver
TWOVIEW_EIGHT_POINT, TWOVIEW_FIVE_POINT = 0, 1
# include/pcs_hip.h PCS_ALIGN_*: per-problem status of the point-set registration, and its models
ALIGN_OK, ALIGN_TOO_FEW, ALIGN_DEGENERATE, ALIGN_NONFINITE, ALIGN_NO_CONSENSUS = 0, 1, 2, 3, 4
ALIGN_MODEL_IDS = {"rigid": 0, "similarity": 1}
# include/pcs_hip.h PCS_IMAP_*: point modes, ray flags, interpolations and image types of the image mapper
IMAP_UNDISTORT, IMAP_DISTORT, IMAP_RAY = 0, 1, 2
IMAP_NORMALISED, IMAP_WORLD, IMAP_NO_DISTORT = 1, 2, 4
IMAP_INTERP_IDS = {"nearest": 0, "bilinear": 1, "bicubic": 2}
IMAP_DTYPE_IDS = {"uint8": 0, "float32": 1}
# include/pcs_hip.h PCS_STEREO_*: status bits of the stereo matcher
STEREO_NOT_STRICT, STEREO_TEXTURE, STEREO_UNIQUENESS, STEREO_LEFT_RIGHT, STEREO_VALIDITY = 1, 2, 4, 8, 16
# include/pcs_hip.h PCS_FUSE_*: status bits of the depth-map fusion and the width of its support word
FUSE_INVALID_DEPTH, FUSE_FEW_VIEWS, FUSE_DUPLICATE, FUSE_MAX_NEIGHBOURS = 1, 2, 4, 32
# include/pcs_hip.h PCS_SWEEP_*: status bits of the plane sweep and its limits
SWEEP_NOT_STRICT, SWEEP_NO_VIEW, SWEEP_UNIQUENESS, SWEEP_MAX_NEIGHBOURS, SWEEP_MAX_PLANES = 1, 2, 4, 16, 1024
# include/pcs_hip.h PCS_PM_*: status values of the PatchMatch depth and its limit
PM_NOT_STRICT, PM_NO_VIEW, PM_MAX_NEIGHBOURS = 1, 2, 16
# include/pcs_hip.h PCS_TSDF_*: the limits of the TSDF volume
TSDF_MAX_DIM, TSDF_MAX_WEIGHT = 1024, 65535
# include/pcs_hip.h PCS_TSDF_RAY_* and PCS_TSDF_RAYCAST_NO_SKIP: per-pixel status of the ray-cast and its flag
TSDF_RAY_HIT, TSDF_RAY_NO_NORMAL, TSDF_RAY_NO_CROSSING, TSDF_RAY_MISSED = 0, 1, 2, 3
TSDF_RAYCAST_NO_SKIP = 1
# include/pcs_hip.h PCS_COLOUR_*: how the contributing views of a point are combined
COLOUR_MODE_IDS = {"blend": 0, "best": 1}
RIGPOSE_RESIDUALS = 1                    # include/pcs_hip.h PCS_RIGPOSE_RESIDUALS
# include/pcs_hip.h PCS_RIGPOSE_*: per-image status of the rig localiser (the meanings of PCS_PNP_*)
RIGPOSE_NOT_ESTIMATED, RIGPOSE_CONVERGED, RIGPOSE_MAX_ITER, RIGPOSE_NO_DECREASE = 0, 1, 2, 3
# include/pcs_hip.h PCS_INTR_MODEL_*, PCS_INTR_* (per camera) and PCS_INTR_GROUP_* (per (camera, image, board) group)
INTR_MODEL_IDS = {"auto": 0, "full": 1, "focal": 2}
INTR_NOT_ESTIMATED, INTR_FULL, INTR_FOCAL, INTR_FOCAL_FALLBACK = 0, 1, 2, 3
INTR_GROUP_TOO_FEW, INTR_GROUP_USED, INTR_GROUP_NOT_PLANAR, INTR_GROUP_NOT_FINITE, INTR_GROUP_FIT_FAILED = 0, 1, 2, 3, 4
# include/pcs_hip.h PCS_STATS_*: the groupings of the residual statistics, in the order of the device's outputs, and the run flag
STATS_GROUPINGS = {"camera": 0, "image": 1, "key": 2, "view": 3, "overall": 4}
STATS_NO_ORDER_STATISTICS = 1


SYMBOLS = {
    "pcs_version": (c_int, []),
    "pcs_last_error": (c_char_p, []),
    "pcs_device_count": (c_int, []),
    "pcs_create": (c_int, [POINTER(_P), c_int, c_int, c_int64, c_int64, c_int64, c_int]),
    "pcs_destroy": (c_int, [_P]),
    "pcs_n_params": (c_int64, [_P]),
    "pcs_row_len": (c_int, [_P]),
    "pcs_n_detections": (c_int64, [_P]),
    "pcs_set_detections_table": (c_int, [_P, POINTER(c_double), c_int64]),
    "pcs_set_detections": (c_int, [_P, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_double), c_int64]),
    "pcs_set_template": (c_int, [_P, POINTER(c_double)]),
    "pcs_eval": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_eval_device": (c_int, [_P, POINTER(c_double), _P, _P, _P]),
    "pcs_eval_device_resident": (c_int, [_P, _P, _P, _P, _P]),
    "pcs_csr_structure": (c_int, [_P, POINTER(c_uint8), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "pcs_block_param_inds": (c_int, [_P, POINTER(c_int64)]),
    "pcs_set_unfixed": (c_int, [_P, POINTER(c_uint8), POINTER(c_int64)]),
    "pcs_eval_compact": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_eval_compact_device": (c_int, [_P, POINTER(c_double), _P, _P, _P]),
    "pcs_legacy_cost": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_linearize": (c_int, [_P, POINTER(c_double)]),
    "pcs_matfree": (c_int, [_P, c_int, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_normal_equations": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_normal_equations_device": (c_int, [_P, POINTER(c_double), c_void_p, c_void_p, c_void_p, c_void_p]),
    "pcs_normal_layout": (c_int, [_P, POINTER(c_int64)]),
    "pcs_normal_blocks_device": (c_int, [_P, _P, _P, _P]),
    "pcs_schur_prepare": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcs_schur_finish": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcs_lm_decide": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcs_lm_trial": (c_int, [_P, _P, _P]),
    "pcs_lm_trial_build": (c_int, [_P, _P, _P]),
    "pcs_lm_trial_finish": (c_int, [_P, _P, _P]),
    "pcs_schur_syrk": (c_int, [c_int, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P]),
    "pcs_schur_vtx": (c_int, [c_int, c_int64, c_int64, _P, c_int64, _P, _P, _P]),
    "pcs_schur_syrk_work_len": (c_int64, [c_int64, c_int64]),
    "pcs_schur_syrk_ordered": (c_int, [c_int, c_int64, c_int64, _P, c_int64, _P, c_int64, _P, _P, _P, c_int64, _P]),
    "pcs_dense_spd_work_len": (c_int64, [c_int64]),
    "pcs_dense_spd_solve": (c_int, [c_int, c_int64, _P, c_int64, _P, _P, _P, _P, _P]),
    "pcs_dense_spd_solve_algo": (c_int, [c_int, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int]),
    "pcs_dense_spd_solve_opts": (c_int, [c_int, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int, c_int64]),
    "pcs_cov_trsm": (c_int, [c_int, c_int64, _P, c_int64, _P, c_int64, c_int64, c_int, _P]),
    "pcs_cov_block_gram": (c_int, [c_int, _P, c_int64, c_int64, c_int64, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_double, _P]),
    "pcs_normal_descriptors": (c_int, [c_int, c_int, c_int, POINTER(c_int32)]),
    "pcs_genchain_create": (c_int, [POINTER(_P), c_char_p, c_int, c_int, c_int, POINTER(c_int64), POINTER(c_int32), c_int, POINTER(c_int64), c_int64, c_int64,
                                    c_int64, c_int64, c_int64, c_int64, c_int, c_int]),
    "pcs_genchain_destroy": (c_int, [_P]),
    "pcs_blockcheck": (c_int, [c_char_p, c_int, c_int, c_int, c_int, c_int, POINTER(c_double), c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_genchain_row_len": (c_int, [_P]),
    "pcs_genchain_set_detections_table": (c_int, [_P, POINTER(c_double), c_int64]),
    "pcs_genchain_set_template": (c_int, [_P, POINTER(c_double)]),
    "pcs_genchain_eval": (c_int, [_P, POINTER(c_double), _P, _P]),
    "pcs_genchain_eval_device": (c_int, [_P, _P, _P, _P, _P]),
    "pcs_genchain_set_one_launch": (c_int, [_P, c_int]),
    "pcs_genchain_set_unfixed": (c_int, [_P, POINTER(c_uint64), POINTER(c_int64), c_int64]),
    "pcs_genchain_eval_compact": (c_int, [_P, POINTER(c_double), _P, _P]),
    "pcs_genchain_eval_compact_device": (c_int, [_P, _P, _P, _P, _P]),
    "pcs_genchain_set_blocks": (c_int, [_P, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_int64)]),
    "pcs_genchain_set_group_maps": (c_int, [_P, c_int, POINTER(c_int32), POINTER(c_void_p), POINTER(c_int64), POINTER(c_int32)]),
    "pcs_genchain_linearize": (c_int, [_P, POINTER(c_double)]),
    "pcs_genchain_matfree": (c_int, [_P, c_int, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_genchain_normal_layout": (c_int, [_P, POINTER(c_int64)]),
    "pcs_genchain_normal_blocks_device": (c_int, [_P, _P, _P, _P]),
    "pcs_genchain_lm_trial": (c_int, [_P, _P, _P]),
    "pcs_genchain_lm_trial_build": (c_int, [_P, _P, _P]),
    "pcs_genchain_lm_trial_finish": (c_int, [_P, _P, _P]),
    "pcs_genchain_set_option": (c_int, [_P, c_char_p, c_int64]),
    "pcs_genchain_schur_prepare": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcs_genchain_schur_finish": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcs_genchain_lm_decide": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcs_genchain_device_buffers": (c_int, [_P, POINTER(_P), POINTER(_P)]),
    "pcs_genchain_synchronize": (c_int, [_P, _P]),
    "pcs_genchain_last_kernel_ms": (c_int, [_P, POINTER(c_float), POINTER(c_float)]),
    "pcs_synchronize": (c_int, [_P, _P]),
    "pcs_last_kernel_ms": (c_int, [_P, POINTER(c_float), POINTER(c_float)]),
    "pcs_kernel_ms_mean": (c_int, [_P, POINTER(c_int64), POINTER(c_float), POINTER(c_float)]),
    "pcs_kernel_ms_samples": (c_int, [_P, c_int64, POINTER(c_float), POINTER(c_float), POINTER(c_int64)]),
    "pcs_normal_entry_map": (c_int, [c_int, c_int, POINTER(c_int32)]),
    "pcs_triangulate": (c_int, [c_int, c_int64, POINTER(c_int32), POINTER(c_double), c_int64, POINTER(c_int64), c_int64,
                                POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_float)]),
    "pcs_tri_create": (c_int, [POINTER(_P), c_int, c_int64]),
    "pcs_tri_destroy": (c_int, [_P]),
    "pcs_tri_set_cameras": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_tri_set_observations": (c_int, [_P, c_int64, POINTER(c_int32), POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_tri_set_observations_device": (c_int, [_P, c_int64, _P, _P, c_int64, _P]),
    "pcs_tri_group_device": (c_int, [_P, c_int64, _P, _P, _P, c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_int32), _P]),
    "pcs_tri_run": (c_int, [_P, _P, _P]),
    "pcs_tri_launch_config": (c_int, [_P, POINTER(c_int32)]),
    "pcs_tri_points": (c_int, [_P, POINTER(c_double)]),
    "pcs_tri_synchronize": (c_int, [_P, _P]),
    "pcs_tri_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_tri_refine": (c_int, [_P, c_int, c_double, c_double, c_double, c_int, _P, _P, _P, _P, _P]),
    "pcs_tri_refined": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_double)]),
    "pcs_tri_set_refine_loss": (c_int, [_P, c_int, c_double]),
    "pcs_tri_get_refine_loss": (c_int, [_P, POINTER(c_int), POINTER(c_double)]),
    "pcs_tri_refine_costs": (c_int, [_P, POINTER(c_double)]),
    "pcs_tri_last_refine_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_tri_set_consensus": (c_int, [_P, c_int, c_double, c_uint64]),
    "pcs_tri_get_consensus": (c_int, [_P, POINTER(c_int), POINTER(c_double), POINTER(c_uint64)]),
    "pcs_tri_consensus_results": (c_int, [_P, POINTER(c_uint8), POINTER(c_int32), POINTER(c_double)]),
    "pcs_pnp_create": (c_int, [POINTER(_P), c_int, c_int64, c_int64]),
    "pcs_pnp_destroy": (c_int, [_P]),
    "pcs_pnp_set_cameras": (c_int, [_P, POINTER(c_double)]),
    "pcs_pnp_set_template": (c_int, [_P, POINTER(c_double)]),
    "pcs_pnp_set_observations": (c_int, [_P, c_int64, POINTER(c_int32), POINTER(c_double), c_int64, POINTER(c_int64), POINTER(c_int32)]),
    "pcs_pnp_run": (c_int, [_P, c_int, c_double, c_double, c_double, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    "pcs_pnp_results": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_double)]),
    "pcs_pnp_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_pnp_set_consensus": (c_int, [_P, c_int, c_int, c_double, c_uint64]),
    "pcs_pnp_get_consensus": (c_int, [_P, POINTER(c_int), POINTER(c_int), POINTER(c_double), POINTER(c_uint64)]),
    "pcs_pnp_consensus_results": (c_int, [_P, POINTER(c_uint8), POINTER(c_int32), POINTER(c_double)]),
    "pcs_twoview_create": (c_int, [POINTER(_P), c_int, c_int64]),
    "pcs_twoview_destroy": (c_int, [_P]),
    "pcs_twoview_set_cameras": (c_int, [_P, POINTER(c_double)]),
    "pcs_twoview_set_correspondences": (c_int, [_P, c_int64, POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int64), POINTER(c_int32)]),
    "pcs_twoview_set_consensus": (c_int, [_P, c_int, c_double, c_uint64]),
    "pcs_twoview_get_consensus": (c_int, [_P, POINTER(c_int), POINTER(c_double), POINTER(c_uint64)]),
    "pcs_twoview_set_solver": (c_int, [_P, c_int, c_int]),
    "pcs_twoview_get_solver": (c_int, [_P, POINTER(c_int), POINTER(c_int)]),
    "pcs_twoview_run": (c_int, [_P, c_int, c_int, c_int, _P, _P]),
    "pcs_twoview_results": (c_int, [_P, POINTER(c_double), POINTER(c_int32), POINTER(c_double), POINTER(c_uint8)]),
    "pcs_twoview_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_align_create": (c_int, [POINTER(_P), c_int]),
    "pcs_align_destroy": (c_int, [_P]),
    "pcs_align_set_points": (c_int, [_P, c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_align_set_consensus": (c_int, [_P, c_int, c_double, c_uint64]),
    "pcs_align_get_consensus": (c_int, [_P, POINTER(c_int), POINTER(c_double), POINTER(c_uint64)]),
    "pcs_align_run": (c_int, [_P, c_int, c_int, c_double, c_int, c_int, _P, _P]),
    "pcs_align_results": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_double), POINTER(c_uint8), POINTER(c_double)]),
    "pcs_align_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_imap_create": (c_int, [POINTER(_P), c_int]),
    "pcs_imap_destroy": (c_int, [_P]),
    "pcs_imap_set_cameras": (c_int, [_P, c_int64, POINTER(c_double), POINTER(c_double)]),
    "pcs_imap_set_view": (c_int, [_P, POINTER(c_double), POINTER(c_double)]),
    "pcs_imap_points": (c_int, [_P, c_int, c_int64, _P, c_int, _P, c_int, c_int, _P, _P]),
    "pcs_imap_rays": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, c_int, _P]),
    "pcs_imap_build_maps": (c_int, [_P, c_int, c_int, c_int, _P, c_int, _P]),
    "pcs_imap_remap": (c_int, [_P, c_int64, POINTER(c_int32), _P, c_int, c_int, c_int, c_int, c_int64, _P, c_int, c_int, c_int64, _P, c_int, c_int64, c_int,
                               POINTER(c_double), _P, _P]),
    "pcs_imap_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_stereo_create": (c_int, [POINTER(_P), c_int]),
    "pcs_stereo_destroy": (c_int, [_P]),
    "pcs_stereo_match": (c_int, [_P, c_int64, c_int, c_int, _P, c_int64, _P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "pcs_stereo_reproject": (c_int, [_P, c_int64, c_int, c_int, _P, c_int, POINTER(c_double), c_int64, c_double, c_double, POINTER(c_double), _P, c_int, _P, _P, _P]),
    "pcs_stereo_compact": (c_int, [_P, c_int64, c_int, c_int, _P, c_int, _P, _P, c_int64, _P, _P, _P, _P]),
    "pcs_stereo_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_stereo_sgm": (c_int, [_P, c_int64, c_int, c_int, _P, c_int64, _P, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "pcs_stereo_set_sgm_workspace": (c_int, [_P, c_int64]),
    "pcs_fuse_create": (c_int, [POINTER(_P), c_int]),
    "pcs_fuse_destroy": (c_int, [_P]),
    "pcs_fuse_set_views": (c_int, [_P, c_int64, c_int, c_int, POINTER(c_double), POINTER(c_double)]),
    "pcs_fuse_set_neighbours": (c_int, [_P, POINTER(c_int32), POINTER(c_int32), c_int64]),
    "pcs_fuse_run": (c_int, [_P, _P, c_int, c_double, c_double, c_int, c_int, POINTER(c_double), _P, c_int, _P, _P, _P, _P, _P, c_int, _P, _P]),
    "pcs_fuse_last_kernel_ms": (c_int, [_P, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "pcs_sweep_create": (c_int, [POINTER(_P), c_int]),
    "pcs_sweep_destroy": (c_int, [_P]),
    "pcs_sweep_set_views": (c_int, [_P, c_int64, c_int, c_int, POINTER(c_double), POINTER(c_double)]),
    "pcs_sweep_set_neighbours": (c_int, [_P, POINTER(c_int32), POINTER(c_int32), c_int64]),
    "pcs_sweep_run": (c_int, [_P, _P, c_int64, POINTER(c_double), c_int64, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, _P, _P]),
    "pcs_sweep_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_pm_create": (c_int, [POINTER(_P), c_int]),
    "pcs_pm_destroy": (c_int, [_P]),
    "pcs_pm_set_views": (c_int, [_P, c_int64, c_int, c_int, POINTER(c_double), POINTER(c_double)]),
    "pcs_pm_set_neighbours": (c_int, [_P, POINTER(c_int32), POINTER(c_int32), c_int64]),
    "pcs_pm_init": (c_int, [_P, _P, c_int64, POINTER(c_double), c_int64, POINTER(c_double), c_int, c_int, c_int, c_int, c_uint64, _P, c_int, c_int, _P, _P, _P]),
    "pcs_pm_iterate": (c_int, [_P, c_int, c_int, _P, c_int64, POINTER(c_double), c_int64, POINTER(c_double), c_int, c_int, c_int, c_int, c_uint64, _P, _P, _P]),
    "pcs_pm_finish": (c_int, [_P, c_int, c_int, c_int, c_int, _P, _P, _P, c_int, _P, _P, _P]),
    "pcs_pm_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_tsdf_create": (c_int, [POINTER(_P), c_int]),
    "pcs_tsdf_destroy": (c_int, [_P]),
    "pcs_tsdf_set_views": (c_int, [_P, c_int64, c_int, c_int, POINTER(c_double), POINTER(c_double)]),
    "pcs_tsdf_set_grid": (c_int, [_P, POINTER(c_double), c_double, c_int, c_int, c_int, c_int]),
    "pcs_tsdf_reset": (c_int, [_P]),
    "pcs_tsdf_integrate": (c_int, [_P, _P, c_int, POINTER(c_int32), c_int64, c_double, _P]),
    "pcs_tsdf_volume_ptrs": (c_int, [_P, POINTER(_P), POINTER(_P)]),
    "pcs_tsdf_extract_count": (c_int, [_P, c_int, POINTER(c_int64), POINTER(c_int64), _P]),
    "pcs_tsdf_extract_write": (c_int, [_P, _P, c_int, _P, _P]),
    "pcs_tsdf_last_kernel_ms": (c_int, [_P, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "pcs_tsdf_raycast": (c_int, [_P, c_int64, c_int, c_int, POINTER(c_double), POINTER(c_double), c_int, c_double, c_double, c_double, _P, c_int, _P, _P, c_int, _P]),
    "pcs_tsdf_raycast_last_kernel_ms": (c_int, [_P, POINTER(c_float), POINTER(c_float)]),
    "pcs_tsdf_raycast_count_samples": (c_int, [_P, _P, _P]),
    "pcs_tsdf_point_normals": (c_int, [_P, c_int64, _P, c_int, c_int, _P, _P, _P]),
    "pcs_tsdf_colour_points": (c_int, [_P, c_int64, _P, c_int, _P, c_int64, c_int, c_int, POINTER(c_double), POINTER(c_double), _P, c_int64, c_int, c_int, _P, c_int, c_double, c_double,
                                       c_int, POINTER(c_double), _P, c_int, _P, _P, _P, _P]),
    "pcs_tsdf_colour_views": (c_int, [_P, c_int64, c_int, c_int, POINTER(c_double), POINTER(c_double), _P, c_int, _P, c_int64, c_int, c_int, POINTER(c_double), POINTER(c_double), _P,
                                      c_int64, c_int, c_int, _P, c_int, c_double, c_double, c_int, POINTER(c_double), _P, c_int, _P, _P, _P, _P]),
    "pcs_tsdf_colour_last_kernel_ms": (c_int, [_P, POINTER(c_float), POINTER(c_float)]),
    "pcs_rigpose_create": (c_int, [POINTER(_P), c_int, c_int64, c_int64]),
    "pcs_rigpose_destroy": (c_int, [_P]),
    "pcs_rigpose_set_cameras": (c_int, [_P, POINTER(c_double)]),
    "pcs_rigpose_set_extrinsics": (c_int, [_P, POINTER(c_double)]),
    "pcs_rigpose_set_template": (c_int, [_P, POINTER(c_double)]),
    "pcs_rigpose_set_observations": (c_int, [_P, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_rigpose_set_start": (c_int, [_P, POINTER(c_double)]),
    "pcs_rigpose_run": (c_int, [_P, c_int, c_double, c_double, c_double, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    "pcs_rigpose_results": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_double), POINTER(c_double)]),
    "pcs_rigpose_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_rigpose_set_loss": (c_int, [_P, c_int, c_double]),
    "pcs_rigpose_get_loss": (c_int, [_P, POINTER(c_int), POINTER(c_double)]),
    "pcs_rigpose_costs": (c_int, [_P, POINTER(c_double)]),
    "pcs_intr_create": (c_int, [POINTER(_P), c_int, c_int64, c_int64]),
    "pcs_intr_destroy": (c_int, [_P]),
    "pcs_intr_set_template": (c_int, [_P, POINTER(c_double)]),
    "pcs_intr_set_observations": (c_int, [_P, c_int64, POINTER(c_int32), POINTER(c_double), c_int64, POINTER(c_int64), POINTER(c_int32)]),
    "pcs_intr_run": (c_int, [_P, c_int, c_int, POINTER(c_double), _P, _P, _P, _P, _P, _P, _P, _P]),
    "pcs_intr_results": (c_int, [_P, POINTER(c_double), POINTER(c_int32), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32),
                                 POINTER(c_double)]),
    "pcs_intr_last_kernel_ms": (c_int, [_P, POINTER(c_float)]),
    "pcs_intr_set_consensus": (c_int, [_P, c_int, c_int, c_double, c_uint64]),
    "pcs_intr_get_consensus": (c_int, [_P, POINTER(c_int), POINTER(c_int), POINTER(c_double), POINTER(c_uint64)]),
    "pcs_intr_consensus_results": (c_int, [_P, POINTER(c_uint8), POINTER(c_int32), POINTER(c_double)]),
    "pcs_rig_create": (c_int, [POINTER(_P), c_int, c_int64, c_int64, c_int64]),
    "pcs_rig_destroy": (c_int, [_P]),
    "pcs_rig_set_cameras": (c_int, [_P, POINTER(c_double)]),
    "pcs_rig_set_template": (c_int, [_P, POINTER(c_double), POINTER(c_double)]),
    "pcs_rig_set_observations": (c_int, [_P, c_int64, POINTER(c_int32), POINTER(c_double), c_int64, POINTER(c_int64), POINTER(c_int32), POINTER(c_int32)]),
    "pcs_rig_set_view_poses": (c_int, [_P, POINTER(c_double)]),
    "pcs_rig_run_edges": (c_int, [_P, _P]),
    "pcs_rig_edges": (c_int, [_P, POINTER(c_int32), POINTER(c_double), POINTER(c_double)]),
    "pcs_rig_set_extrinsics": (c_int, [_P, POINTER(c_double)]),
    "pcs_rig_run_scores": (c_int, [_P, _P]),
    "pcs_rig_results": (c_int, [_P, POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_rig_last_kernel_ms": (c_int, [_P, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "pcs_stats_create": (c_int, [POINTER(_P), c_int, c_int64, c_int64, c_int64]),
    "pcs_stats_destroy": (c_int, [_P]),
    "pcs_stats_set_groups": (c_int, [_P, c_int64, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "pcs_stats_set_groups_device": (c_int, [_P, c_int64, _P, _P, _P]),
    "pcs_stats_run": (c_int, [_P, _P, c_int, _P, _P, _P, _P]),
    "pcs_stats_results": (c_int, [_P, c_int, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32), POINTER(c_double), POINTER(c_double), POINTER(c_double),
                                  POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double)]),
    "pcs_stats_errors": (c_int, [_P, POINTER(c_double)]),
    "pcs_stats_last_kernel_ms": (c_int, [_P, POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "pcs_host_alloc": (c_int, [POINTER(_P), c_int64]),
    "pcs_host_free": (c_int, [_P]),
    "pcs_membench": (c_int, [c_int, c_int, c_int64, c_int, c_int, POINTER(c_float)]),
    "pcs_set_option": (c_int, [_P, c_char_p, c_int64]),
    "pcs_set_loss": (c_int, [_P, c_int, c_double]),
    "pcs_get_loss": (c_int, [_P, POINTER(c_int), POINTER(c_double)]),
    "pcs_set_weights": (c_int, [_P, POINTER(c_double), c_int64]),
    "pcs_get_weights": (c_int, [_P, POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_set_prior": (c_int, [_P, POINTER(c_double), POINTER(c_double), c_int64]),
    "pcs_get_prior": (c_int, [_P, POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_prior_add_device": (c_int, [_P, _P, _P, _P]),
    "pcs_genchain_set_prior": (c_int, [_P, POINTER(c_double), POINTER(c_double), c_int64]),
    "pcs_genchain_get_prior": (c_int, [_P, POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_genchain_prior_add_device": (c_int, [_P, _P, _P, _P]),
    "pcs_set_bounds": (c_int, [_P, POINTER(c_double), POINTER(c_double), c_int64]),
    "pcs_get_bounds": (c_int, [_P, POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_bounds_trials": (c_int, [_P, POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_bounds_active_device": (c_int, [_P, _P, _P, _P, _P, _P]),
    "pcs_bounds_truncate_device": (c_int, [_P, _P, _P, _P, _P, _P]),
    "pcs_lm_decide_bounded": (c_int, [_P] * 13),
    "pcs_bounds_active_sel_device": (c_int, [_P] * 9),
    "pcs_bounds_truncate_sel_device": (c_int, [_P] * 7),
    "pcs_genchain_set_bounds": (c_int, [_P, POINTER(c_double), POINTER(c_double), c_int64]),
    "pcs_genchain_get_bounds": (c_int, [_P, POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_genchain_bounds_trials": (c_int, [_P, POINTER(c_double), c_int64, POINTER(c_int64)]),
    "pcs_genchain_bounds_active_device": (c_int, [_P, _P, _P, _P, _P, _P]),
    "pcs_genchain_bounds_truncate_device": (c_int, [_P, _P, _P, _P, _P, _P]),
    "pcs_genchain_lm_decide_bounded": (c_int, [_P] * 13),
    "pcs_device_buffers": (c_int, [_P, POINTER(_P), POINTER(_P)]),
}


class PcsError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"pcs error {code}: {message}")
        self.code = code


_lib = None


def lib() -> ctypes.CDLL:
    """Load libpcs_hip.so (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise OSError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                f"(python -c 'import __graft_entry__ as g; g.build()' or python -m pycamset_amd.build). "
                f"pycamset_amd has no CPU fallback."
            )
        # PyTorch-ROCm wheels bundle their own libamdhip64.so / libhsa-runtime64.so under the same
        # SONAMEs as /opt/rocm's.  Two HIP runtimes in one process cannot both own the GPU, so the
        # runtime torch ships must be the one already loaded when libpcs_hip.so resolves its
        # DT_NEEDED entries: import torch first (set PCS_NO_TORCH=1 for a torch-free process).
        if os.environ.get("PCS_NO_TORCH", "0") != "1":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        handle = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(code: int) -> None:
    if code != PCS_OK:
        raise PcsError(code, (lib().pcs_last_error() or b"").decode("utf-8", "replace"))
