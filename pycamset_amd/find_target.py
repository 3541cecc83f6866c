"""Mirror of pyCamSet/optimisation/find_target.py: where is the known target in new images of a calibrated rig?

    find_target_pose_at_timestep(images, target, cameras) -> pose           ft:9-47
    find_target_poses(image_seq, target, cameras) -> poses                  ft:50-82

The reference detects the target in the images, fixes every camera's "ext" / "int" / "dst" (ft:31-34, :66-69) and runs the whole
bundle adjustment for the poses that are left (ft:36-47, :71-82).  With every camera fixed that is one independent 6-parameter problem
per image, which the device solves in one launch (``compiled_helpers.localise_target``, include/pcs_hip.h pcs_rigpose_run).

On the library's array conventions: detection in images and ``CameraSet`` objects are out of scope, so both functions take the
detections (a ``TargetDetection`` or the flattened (N, 5) table [cam, im, key, u, v]), the template ``points`` (K, 3) or
``target.point_data``, ``intr`` (C, 9) rows [fx, cx, fy, cy, k0, k1, p0, p1, k2] and ``ext`` (C, 3, 4) world -> camera, and return slabs."""
from __future__ import annotations

import numpy as np

from . import compiled_helpers as ch
from .detections import TargetDetection


def _table(detection_or_dct, points):
    """-> (flattened table (N, 5), template (K, 3), images stated by the detection or None)."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim < 2 or pts.shape[-1] != 3:
        raise ValueError("expected template points (..., 3)")
    if isinstance(detection_or_dct, TargetDetection):
        flat = detection_or_dct.return_flattened_keys(pts.shape[:-1])
        data = flat.get_data()
        return (np.empty((0, 5)) if data is None else data), pts.reshape(-1, 3), int(flat.max_ims)
    d = np.asarray(detection_or_dct, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 5:
        raise ValueError("expected a TargetDetection or the flattened table (N, 5) = [cam, im, key, u, v]")
    return d, pts.reshape(-1, 3), None


def find_target_poses(detection_or_dct, points, intr, ext, *, start: str = "pnp", **opts) -> ch.ImagePoses:
    """The target pose of every image (ft:50-82) -> ``compiled_helpers.ImagePoses``; ``opts`` are ``localise_target``'s
    (``n_imgs``, ``poses_init``, ``min_points``, ``max_iter``, ``ftol``, ``xtol``, ``gtol``, ``group_lanes``, ``return_residuals``,
    ``device``, and ``loss`` / ``f_scale``: the robust loss the reference's ``least_squares`` call carries commented out).

    ``start``: where the solve begins when ``poses_init`` is not given.  ``"pnp"`` (default) is ``localise_target``'s own start, the
    best per-view PnP candidate (``compiled_helpers.rig_pose_start``); ``"triangulation"`` registers the template onto the features
    that two or more cameras triangulate (``compiled_helpers.rig_pose_start_3d``): no planar ambiguity, for rigs whose cameras overlap."""
    if start not in ("pnp", "triangulation"):
        raise ValueError(f"start must be 'pnp' or 'triangulation', got {start!r}")
    d, pts, stated = _table(detection_or_dct, points)
    if stated is not None:
        opts.setdefault("n_imgs", stated)
    if start == "triangulation" and opts.get("poses_init") is None and d.shape[0]:
        n_imgs = opts.get("n_imgs")
        n_imgs = int(d[:, 1].max()) + 1 if n_imgs is None else int(n_imgs)
        opts["poses_init"] = ch.rig_pose_start_3d(d, pts, intr, ext, n_imgs, min_points=opts.get("min_points", 6), device=opts.get("device", 0))
    return ch.localise_target(d, pts, intr, ext, **opts)


def find_target_pose_at_timestep(detection_or_dct, points, intr, ext, im_num: int = 0, **opts):
    """The target pose of ONE image (ft:9-47: the detections of a single time step) -> (pose (6,), rms, status).  ``im_num`` selects the
    image of the table (the reference files every detection under image 0, ft:29); ``poses_init``, if given, is the (6,) start;
    ``loss`` / ``f_scale`` as in ``find_target_poses``."""
    if isinstance(im_num, bool) or not isinstance(im_num, (int, np.integer)) or im_num < 0:
        raise ValueError(f"im_num must be an integer >= 0, got {im_num!r}")
    if "n_imgs" in opts:
        raise ValueError("find_target_pose_at_timestep localises one image: n_imgs is not an option")
    d, pts, _ = _table(detection_or_dct, points)
    rows = d[d[:, 1] == im_num].copy()
    rows[:, 1] = 0.0
    if opts.get("poses_init") is not None:
        opts["poses_init"] = np.asarray(opts["poses_init"], dtype=np.float64).reshape(1, 6)
    res = ch.localise_target(rows, pts, intr, ext, n_imgs=1, **opts)
    return res.poses[0], float(res.rms[0]), int(res.status[0])
