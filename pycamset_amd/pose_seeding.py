"""From per-view target poses to a start of the calibration: the NumPy mirror of ``estimate_camera_relative_poses``
(pyCamSet optimisation/template_handler.py:468-601) on top of the device's batched PnP (``compiled_helpers.estimate_view_poses``,
in place of cv2.solvePnPGeneric per view, calibration_targets/abstract_target.py:345-405) and the device's legacy cost
(``compiled_helpers.bundle_adjustment_costfn``).

Frames, as in the reference: a view transform M[c, i] takes target coordinates to camera c in image i.  The world is the target of the
reference pose: the extrinsics of camera c are M[c, ref_pose], and camera c's estimate of the target pose of image i is
inv(M[c, ref_pose]) M[c, i].  Per image the estimate with the lowest legacy cost over ALL of the image's detections is kept.

One deviation on purpose: the reference appends the final per-image costs to the last camera's list (th:594-595) and so returns
2 I values; this returns the I final ones."""
from __future__ import annotations

import numpy as np
from scipy.spatial.transform import Rotation


def pose_to_4x4(p: np.ndarray) -> np.ndarray:
    """(..., 6) [rotvec, t] -> (..., 4, 4); NaN poses give NaN matrices."""
    p = np.asarray(p, dtype=np.float64)
    flat = p.reshape(-1, 6)
    out = np.full((flat.shape[0], 4, 4), np.nan)
    ok = np.all(np.isfinite(flat), axis=1)
    if np.any(ok):
        out[ok] = 0.0
        out[ok, :3, :3] = Rotation.from_rotvec(flat[ok, :3]).as_matrix()
        out[ok, :3, 3] = flat[ok, 3:]
        out[ok, 3, 3] = 1.0
    return out.reshape(p.shape[:-1] + (4, 4))


def pose_from_4x4(M: np.ndarray) -> np.ndarray:
    """(..., 4, 4) -> (..., 6) [rotvec, t] (general_utils.ext_4x4_to_rod); NaN matrices give NaN poses."""
    M = np.asarray(M, dtype=np.float64)
    flat = M.reshape(-1, 4, 4)
    out = np.full((flat.shape[0], 6), np.nan)
    ok = np.all(np.isfinite(flat.reshape(flat.shape[0], -1)), axis=1)
    if np.any(ok):
        out[ok, :3] = Rotation.from_matrix(flat[ok, :3, :3]).as_rotvec()
        out[ok, 3:] = flat[ok, :3, 3]
    return out.reshape(M.shape[:-2] + (6,))


def check_feasiblity_and_update_refpose(Mat_ac: np.ndarray, ref_pose: int) -> int:
    """th:454-466: ``ref_pose`` when every camera has a transform for it, else the first image every camera sees; ValueError when
    there is none."""
    missing = np.isnan(Mat_ac[:, :, 0, 0])
    visible_pose = ~np.any(missing, axis=0)
    if visible_pose.shape[0] and visible_pose[ref_pose]:
        return int(ref_pose)
    if not np.any(visible_pose):
        raise ValueError("Couldn't find an initial pose for all cameras.")
    return int(np.argmax(visible_pose))


def intrinsic_matrices(intr: np.ndarray) -> np.ndarray:
    """(C, 9) slab rows -> (C, 3, 3) camera matrices."""
    K = np.zeros((intr.shape[0], 3, 3))
    K[:, 0, 0], K[:, 0, 2], K[:, 1, 1], K[:, 1, 2], K[:, 2, 2] = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 1.0
    return K


def estimate_camera_relative_poses(dct, points, intr, n_cams: int, n_imgs: int, ref_cam: int = 0, ref_pose: int = 0, *, view_pose_fn=None,
                                   cost_fn=None):
    """-> (extr (C, 6), poses (I, 6), per_im_error (I,), missing (I,) bool).

    ``dct`` (N, 5) flattened detections, ``points`` (K, 3) template, ``intr`` (C, 9).  ``view_pose_fn(dct, points, intr, n_imgs=...)``
    returns an object with ``poses`` (C, I, 6) (default: the device's ``estimate_view_poses``); ``cost_fn`` has the signature of
    ``bundle_adjustment_costfn`` (default: the device's).  ``ref_cam`` is accepted for the reference's signature; as there, the world
    frame is the target of the reference pose, whichever camera is named.  ``missing[i]``: no camera estimated image i."""
    from . import compiled_helpers as ch

    view_pose_fn = ch.estimate_view_poses if view_pose_fn is None else view_pose_fn
    cost_fn = ch.bundle_adjustment_costfn if cost_fn is None else cost_fn
    dct = np.ascontiguousarray(dct, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    intr = np.asarray(intr, dtype=np.float64)
    if intr.shape != (n_cams, 9):
        raise ValueError(f"expected intr ({n_cams}, 9)")
    view_poses = np.asarray(view_pose_fn(dct, points, intr, n_imgs=n_imgs).poses, dtype=np.float64)
    if view_poses.shape != (n_cams, n_imgs, 6):
        raise ValueError(f"view_pose_fn must return poses ({n_cams}, {n_imgs}, 6)")
    Mat_ac = pose_to_4x4(view_poses)                                         # th:484-491
    missing = np.all(np.isnan(Mat_ac[:, :, 0, 0]), axis=0)
    ref_pose = check_feasiblity_and_update_refpose(Mat_ac, ref_pose)         # th:493
    Mrt_ac = Mat_ac[:, ref_pose].copy()                                      # th:497: the extrinsics
    Mat_rt_ac = np.linalg.inv(Mrt_ac)[:, None] @ Mat_ac                      # th:499-502: camera c's estimate of every target pose
    K = intrinsic_matrices(intr)
    dists = np.ascontiguousarray(intr[:, 4:9])
    proj = K @ Mrt_ac[:, :3, :]                                              # th:508
    im_of_row = dct[:, 1].astype(np.int64)

    def per_image_cost(M_rt):                                                # th:535-560
        imlocs = np.einsum("iab,kb->ika", M_rt[:, :3, :3], points) + M_rt[:, None, :3, 3]
        costs = np.asarray(cost_fn(dct, imlocs, proj, K, dists), dtype=np.float64)
        costs = np.sqrt(np.sum(costs.reshape(-1, 2) ** 2, axis=1))
        return np.bincount(im_of_row, weights=costs, minlength=n_imgs)[:n_imgs]

    errors = np.empty((n_cams, n_imgs))
    for c in range(n_cams):
        M_c = Mat_rt_ac[c]
        nanform = np.isnan(M_c[:, 0, 0])
        for i in range(n_imgs):                                              # th:528-532: forward fill
            if nanform[i]:
                if i == 0:
                    raise ValueError("No pose in first image")
                M_c[i] = M_c[i - 1]
        errors[c] = per_image_cost(M_c)
    estimate_locs = np.argmin(errors, axis=0)                                # th:578
    Mat_rt = Mat_rt_ac[estimate_locs, np.arange(n_imgs)]                     # th:582
    per_im_error = per_image_cost(Mat_rt)                                    # th:585-595
    Mat_rt[ref_pose] = np.eye(4)                                             # th:600
    return pose_from_4x4(Mrt_ac), pose_from_4x4(Mat_rt), per_im_error, missing
