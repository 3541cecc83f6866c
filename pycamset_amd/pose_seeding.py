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

import functools
from dataclasses import dataclass

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


def default_view_pose_fn(view_pose_fn, view_consensus: int):
    """The ``view_pose_fn`` of the seedings: the caller's, or the device's ``estimate_view_poses`` — with ``view_consensus`` > 0 its
    consensus sampling with that many hypotheses (``functools.partial(estimate_view_poses, consensus=...)``; a caller who wants other
    ``sample_size`` / ``inlier_px`` / ``seed`` passes such a partial as ``view_pose_fn`` itself)."""
    from . import compiled_helpers as ch

    if view_pose_fn is not None:
        if view_consensus:
            raise ValueError("view_consensus goes with the default view_pose_fn; bind the keyword into your own with functools.partial")
        return view_pose_fn
    n_hyp = ch.check_consensus_options(view_consensus, 6, 8.0, 0)[0]
    return functools.partial(ch.estimate_view_poses, consensus=n_hyp) if n_hyp else ch.estimate_view_poses


def estimate_camera_relative_poses(dct, points, intr, n_cams: int, n_imgs: int, ref_cam: int = 0, ref_pose: int = 0, *, view_pose_fn=None,
                                   cost_fn=None, view_consensus: int = 0):
    """-> (extr (C, 6), poses (I, 6), per_im_error (I,), missing (I,) bool).

    ``dct`` (N, 5) flattened detections, ``points`` (K, 3) template, ``intr`` (C, 9).  ``view_pose_fn(dct, points, intr, n_imgs=...)``
    returns an object with ``poses`` (C, I, 6) (default: the device's ``estimate_view_poses``); ``cost_fn`` has the signature of
    ``bundle_adjustment_costfn`` (default: the device's).  ``ref_cam`` is accepted for the reference's signature; as there, the world
    frame is the target of the reference pose, whichever camera is named.  ``missing[i]``: no camera estimated image i.
    ``view_consensus`` > 0: the default ``view_pose_fn`` with that many consensus hypotheses per view (``default_view_pose_fn``)."""
    from . import compiled_helpers as ch

    view_pose_fn = default_view_pose_fn(view_pose_fn, view_consensus)
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


# ---- seeding over the co-visibility graph: no image has to be seen by every camera --------------------------------------------------
def rigid_inverse(M: np.ndarray) -> np.ndarray:
    """(..., 4, 4) rigid transforms -> their inverses [R' | -R' t]."""
    out = np.zeros_like(M)
    Rt = np.swapaxes(M[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum("...ab,...b->...a", Rt, M[..., :3, 3])
    out[..., 3, 3] = 1.0
    return out


def to_4x4(T: np.ndarray) -> np.ndarray:
    """(..., 3, 4) -> (..., 4, 4) with the row [0, 0, 0, 1] (NaN transforms stay NaN in their first three rows)."""
    out = np.zeros(T.shape[:-2] + (4, 4))
    out[..., :3, :] = T
    out[..., 3, 3] = 1.0
    return out


def relative_gap(best: np.ndarray, runner_up: np.ndarray) -> np.ndarray:
    """(runner-up - best) / runner-up: how clearly an argmin was decided; inf where there is no runner-up, 0 where both vanish."""
    best, runner_up = np.asarray(best, dtype=np.float64), np.asarray(runner_up, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(runner_up > 0, (runner_up - best) / runner_up, 0.0)
    return np.where(np.isfinite(runner_up), gap, np.inf)


def shortest_path_tree(n_cams: int, pairs: np.ndarray, cost: np.ndarray, ref_cam: int):
    """Dijkstra from ``ref_cam`` over the undirected edges ``pairs`` (P, 2) of finite ``cost`` (P,) -> (parents (C,), -1 for ``ref_cam``
    and for unreachable cameras; the reached cameras in the order they were settled).  Among equally distant cameras the lower index is
    settled first, among equally good parents the lower index is kept."""
    w = np.full((n_cams, n_cams), np.inf)
    ok = np.isfinite(cost)
    w[pairs[ok, 0], pairs[ok, 1]] = w[pairs[ok, 1], pairs[ok, 0]] = cost[ok]
    dist = np.full(n_cams, np.inf)
    dist[ref_cam] = 0.0
    parents = np.full(n_cams, -1, dtype=np.int64)
    done = np.zeros(n_cams, dtype=bool)
    settled = []
    for _ in range(n_cams):
        u = int(np.argmin(np.where(done, np.inf, dist)))   # the first of equal minima: the lowest index
        if done[u] or not np.isfinite(dist[u]):
            break
        done[u] = True
        settled.append(u)
        nd = dist[u] + w[u]
        better = ~done & ((nd < dist) | ((nd == dist) & np.isfinite(nd) & (u < parents)))
        dist[better], parents[better] = nd[better], u
    return parents, settled


@dataclass
class RigGraphInfo:
    """Diagnostics of ``estimate_camera_relative_poses_graph``: per camera pair a < b (``pairs`` (P, 2), lexicographic) the number of
    shared images ``n``, the ``medoid`` image, the spread ``sigma`` and the relative ``gap`` between the medoid's score and the
    runner-up's, the transform ``T`` (P, 3, 4) and the tree cost ``edge_cost`` = sigma + rho / n; the tree's ``parents`` (C,) (-1 for
    ``ref_cam``); per image ``best_cam`` (-1: missing) and ``error_gap``, the relative gap between the lowest and the second lowest
    candidate error; the full ``errors`` (C, I) matrix (NaN: camera c has no estimate of image i); ``dependent`` (C, I): image i is
    the medoid image of the edge from camera c to its parent, where c's estimate repeats the parent's and is no candidate; ``rho``."""
    pairs: np.ndarray
    n: np.ndarray
    medoid: np.ndarray
    sigma: np.ndarray
    gap: np.ndarray
    T: np.ndarray
    edge_cost: np.ndarray
    parents: np.ndarray
    best_cam: np.ndarray
    error_gap: np.ndarray
    errors: np.ndarray
    dependent: np.ndarray
    rho: float


def estimate_camera_relative_poses_graph(dct, points, intr, n_cams: int, n_imgs: int, ref_cam: int = 0, ref_pose: int = 0, *, view_pose_fn=None,
                                         edge_fn=None, score_fn=None, return_graph: bool = False, view_consensus: int = 0):
    """-> (extr (C, 6), poses (I, 6), per_im_error (I,), missing (I,) bool) like ``estimate_camera_relative_poses``, for any rig whose
    co-visibility graph is connected: no image has to be seen by every camera.

    1. Per camera pair the relative transform is the medoid of M[a, i] inv(M[b, i]) over the images i both cameras have a pose for
       (``edge_fn(view_poses, points)`` -> an object with the fields of ``compiled_helpers.EdgeConsensus``; default: the device's).
    2. The extrinsics are composed along the shortest-path tree from ``ref_cam`` with edge cost sigma + rho / n (``shortest_path_tree``):
       E_ref_cam = I, E_c = T[c, parent] E_parent.  Cameras the tree does not reach raise ValueError naming them.
    3. Every camera's estimate W[c', i] = inv(E_c') M[c', i] of every image's target pose is scored over all detections of the image
       (``score_fn(dct, points, intr, view_poses, ext (C, 3, 4), n_imgs)`` -> (W (C, I, 3, 4), errors (C, I)); default: the device's); the
       image takes the candidate of lowest finite error, ties to the lowest camera.  Camera c is no candidate for the medoid image of the
       edge to its parent: E_c is made from that very view, so its estimate there repeats the parent's and their errors tie up to
       rounding by construction.  An image without a finite candidate is ``missing``
       and takes the pose of the previous non-missing image (of the first one, when none precedes it).
    4. The world becomes the target of ``ref_pose`` (of the first non-missing image, when that one is missing): that pose is exactly 0.

    ``per_im_error`` is NaN for missing images.  ``return_graph=True`` appends a ``RigGraphInfo``.  ``view_consensus`` > 0: the default
    ``view_pose_fn`` with that many consensus hypotheses per view (``default_view_pose_fn``): the medoid of step 1 protects an edge
    against a wrong VIEW, the consensus repairs a view that holds wrong detections."""
    from . import compiled_helpers as ch

    view_pose_fn = default_view_pose_fn(view_pose_fn, view_consensus)
    edge_fn = ch.rig_edge_consensus if edge_fn is None else edge_fn
    score_fn = ch.rig_candidate_scores if score_fn is None else score_fn
    dct = np.ascontiguousarray(dct, dtype=np.float64)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    intr = np.asarray(intr, dtype=np.float64)
    C, I = int(n_cams), int(n_imgs)
    if intr.shape != (C, 9):
        raise ValueError(f"expected intr ({C}, 9)")
    if not 0 <= int(ref_cam) < C or not 0 <= int(ref_pose) < I:
        raise ValueError(f"ref_cam must be in [0, {C}) and ref_pose in [0, {I})")
    view_poses = np.asarray(view_pose_fn(dct, points, intr, n_imgs=I).poses, dtype=np.float64)
    if view_poses.shape != (C, I, 6):
        raise ValueError(f"view_pose_fn must return poses ({C}, {I}, 6)")
    # 1. edges
    edges = edge_fn(view_poses, points)
    pairs, n = np.asarray(edges.pairs, dtype=np.int64).reshape(-1, 2), np.asarray(edges.n, dtype=np.int64)
    sigma, T = np.asarray(edges.sigma, dtype=np.float64), to_4x4(np.asarray(edges.T, dtype=np.float64).reshape(-1, 3, 4))
    usable = (n > 0) & (np.asarray(edges.medoid) >= 0) & np.isfinite(sigma)
    with np.errstate(divide="ignore", invalid="ignore"):
        edge_cost = np.where(usable, sigma + float(edges.rho) / np.maximum(n, 1), np.inf)
    # 2. tree
    parents, settled = shortest_path_tree(C, pairs, edge_cost, int(ref_cam))
    lost = sorted(set(range(C)) - set(settled))
    if lost:
        raise ValueError(f"Couldn't find an initial pose for all cameras: cameras {lost} share no estimated image with the cameras connected to camera {int(ref_cam)}.")
    E = np.zeros((C, 4, 4))
    E[int(ref_cam)] = np.eye(4)
    medoid = np.asarray(edges.medoid, dtype=np.int64)
    # E_c is made of camera c's and its parent's views of the edge's medoid image, so W[c, medoid] IS W[parent, medoid] up to rounding:
    # there camera c is no candidate of its own (its error ties with the parent's by construction, and rounding would pick)
    dependent = np.zeros((C, I), dtype=bool)
    for c in settled[1:]:
        p = int(parents[c])
        a, b = min(c, p), max(c, p)
        T_ab = T[a * (2 * C - a - 1) // 2 + b - a - 1]                        # camera b -> camera a
        E[c] = (T_ab if c == a else rigid_inverse(T_ab)) @ E[p]
        dependent[c, medoid[a * (2 * C - a - 1) // 2 + b - a - 1]] = True
    # 3. candidates
    W, errors = score_fn(dct, points, intr, view_poses, E[:, :3, :], I)
    W, errors = to_4x4(np.asarray(W, dtype=np.float64).reshape(C, I, 3, 4)), np.asarray(errors, dtype=np.float64).reshape(C, I)
    finite = np.isfinite(errors) & ~dependent
    ranked = np.sort(np.where(finite, errors, np.inf), axis=0)
    missing = ~finite.any(axis=0)
    if missing.all():
        raise ValueError("No image has an estimated target pose.")
    best_cam = np.where(missing, -1, np.argmin(np.where(finite, errors, np.inf), axis=0))
    per_im_error = np.where(missing, np.nan, ranked[0])
    error_gap = relative_gap(ranked[0], ranked[1]) if C > 1 else np.full(I, np.inf)
    pose = W[np.maximum(best_cam, 0), np.arange(I)]
    first = int(np.argmin(missing))
    for i in range(I):
        if missing[i]:
            pose[i] = pose[i - 1] if i > first else pose[first]
    # 4. the world is the target of the reference pose
    ref = int(ref_pose) if not missing[int(ref_pose)] else first
    P_ref = pose[ref].copy()
    pose = rigid_inverse(P_ref) @ pose
    E = E @ P_ref
    poses6 = pose_from_4x4(pose)
    poses6[ref] = 0.0
    out = (pose_from_4x4(E), poses6, per_im_error, missing)
    if not return_graph:
        return out
    info = RigGraphInfo(pairs=pairs, n=n, medoid=medoid, sigma=sigma, dependent=dependent,
                        gap=relative_gap(edges.score, edges.runner_up), T=T[:, :3, :], edge_cost=edge_cost, parents=parents, best_cam=best_cam,
                        error_gap=error_gap, errors=errors, rho=float(edges.rho))
    return out + (info,)


# ---- resection: the extrinsics of every camera with the target poses held fixed ----------------------------------------------------
@dataclass
class CameraResection:
    """What ``resect_cameras`` returns, per camera: ``poses`` (C, 6) = [rotvec, t] world -> camera (NaN where not estimated), ``rms`` /
    ``rms_init`` (C,) RMS reprojection error in pixels, ``status`` (PNP_*), ``iterations``, ``n_points`` (C,) int32; ``images`` (I,)
    bool: the images that took part (a finite pose)."""
    poses: np.ndarray
    rms: np.ndarray
    rms_init: np.ndarray
    status: np.ndarray
    iterations: np.ndarray
    n_points: np.ndarray
    images: np.ndarray


def resect_cameras(dct, points, intr, image_poses, *, view_pose_fn=None, **opts) -> CameraResection:
    """The mirror problem of ``compiled_helpers.localise_target``: the extrinsics of every camera with the target poses of the images
    held fixed — a camera added to a calibrated rig.  No kernel of its own: the world points T_i X_k of all images form one "template"
    of I * K points with key' = i * K + k, every camera is one view of it, and the batched PnP
    (``view_pose_fn(dct', points', intr, n_imgs=1, **opts)``, default ``compiled_helpers.estimate_view_poses``) does the rest.
    ``image_poses`` (I, 6) = [rotvec, t], target -> world; images with a NaN pose are dropped from the table first.  ``opts`` reach
    ``estimate_view_poses`` as they are: ``consensus=64`` (with ``sample_size``, ``inlier_px``, ``seed``) resects every camera from
    the consensus of its detections, so that a few wrong ids do not bend the new camera."""
    from . import compiled_helpers as ch

    view_pose_fn = ch.estimate_view_poses if view_pose_fn is None else view_pose_fn
    d = np.asarray(dct, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    K = np.asarray(intr, dtype=np.float64)
    P = np.asarray(image_poses, dtype=np.float64)
    if d.ndim != 2 or d.shape[1] != 5 or K.ndim != 2 or K.shape[1] != 9 or P.ndim != 2 or P.shape[1] != 6:
        raise ValueError("expected dct (N, 5) = [cam, im, key, u, v], intr (C, 9) and image poses (I, 6)")
    C, I, nk = K.shape[0], P.shape[0], pts.shape[0]
    if d.shape[0] and (d[:, 0].min() < 0 or d[:, 0].max() >= C or d[:, 1].min() < 0 or d[:, 1].max() >= I or d[:, 2].min() < 0 or d[:, 2].max() >= nk):
        raise ValueError("camera, image or key index of the table outside the intrinsics / image poses / template")
    known = np.all(np.isfinite(P), axis=1)
    T = pose_to_4x4(np.where(known[:, None], P, 0.0))
    world = (np.einsum("iab,kb->ika", T[:, :3, :3], pts) + T[:, None, :3, 3]).reshape(I * nk, 3)   # unknown images: never referenced
    rows = d[known[d[:, 1].astype(np.int64)]]
    table = np.empty((rows.shape[0], 5))
    table[:, 0], table[:, 1] = rows[:, 0], 0.0
    table[:, 2] = rows[:, 1].astype(np.int64) * nk + rows[:, 2].astype(np.int64)
    table[:, 3:] = rows[:, 3:]
    vp = view_pose_fn(table, world, K, n_imgs=1, **opts)
    col = lambda name, fill, dtype: (np.asarray(getattr(vp, name))[:, 0] if hasattr(vp, name) else np.full(C, fill)).astype(dtype)   # noqa: E731
    return CameraResection(poses=np.asarray(vp.poses, dtype=np.float64).reshape(C, 6), rms=col("rms", np.nan, np.float64),
                           rms_init=col("rms_init", np.nan, np.float64), status=col("status", 0, np.int32),
                           iterations=col("iterations", 0, np.int32), n_points=col("n_points", 0, np.int32), images=known)


# ---- target-free seeding: incremental reconstruction from the detections alone ------------------------------------
@dataclass
class SceneSeed:
    """What ``seed_scene`` returns.  ``extr`` (C, 6) = [rotvec, t] world -> camera, NaN for a camera that was not placed; ``points``
    (K, 3), NaN where not triangulated; ``placed`` (C,) bool; ``round_of_camera`` (C,) int: 0 for the first pair, r for a camera
    resected in round r, -1 for one never placed; ``n_views`` (K,) placed cameras a point was triangulated from and ``rms`` (K,) its RMS
    reprojection error in pixels; ``first_pair`` (a, b); ``frame_cam``: the camera whose frame is the world — ``ref_cam`` when it was
    placed, else the first pair's camera a; ``two_view``: the ``TwoViewResult`` of all pairs."""
    extr: np.ndarray
    points: np.ndarray
    placed: np.ndarray
    round_of_camera: np.ndarray
    n_views: np.ndarray
    rms: np.ndarray
    first_pair: tuple
    frame_cam: int
    two_view: object


def _triangulate_placed(seen, M, K, placed, n_keys, triangulate_fn, tri_opts):
    """Every key that at least two placed cameras see, through ``refine_triangulation``: (points (n_keys, 3), n_views, rms), NaN / 0 elsewhere."""
    cams = np.nonzero(placed)[0]
    rows = np.concatenate([np.column_stack([np.full(seen[c][0].shape[0], c, dtype=np.float64), seen[c][0], seen[c][1]]) for c in cams])
    rows = rows[np.lexsort((rows[:, 0], rows[:, 1]))]   # by key, then camera
    count = np.bincount(rows[:, 1].astype(np.int64), minlength=n_keys)
    rows = rows[count[rows[:, 1].astype(np.int64)] >= 2]
    points, n_views, rms = np.full((n_keys, 3), np.nan), np.zeros(n_keys, dtype=np.int32), np.full(n_keys, np.nan)
    if rows.shape[0] == 0:
        return points, n_views, rms
    keys = rows[:, 1].astype(np.int64)
    head = np.ones(keys.shape[0], dtype=bool)
    head[1:] = keys[1:] != keys[:-1]
    start = np.concatenate([np.nonzero(head)[0], [keys.shape[0]]]).astype(np.int64)
    Km = intrinsic_matrices(K)
    Mp = np.where(placed[:, None, None], M, np.eye(4))   # a camera that is not placed is never referenced
    res = triangulate_fn(rows[:, [0, 2, 3]], Km @ Mp[:, :3, :], start, Km, K[:, 4:9], **tri_opts)
    ok = np.all(np.isfinite(res.points), axis=1)
    k = keys[head][ok]
    points[k], n_views[k], rms[k] = res.points[ok], np.asarray(res.n_views)[ok], np.asarray(res.rms)[ok]
    return points, n_views, rms


def seed_scene(dct, intr, n_cams: int, *, ref_cam: int = 0, baseline: float = 1.0, consensus: int = 64, inlier_px: float = 2.0, seed: int = 0,
               min_points: int = 16, resect_opts: dict | None = None, tri_opts: dict | None = None, two_view_fn=None, triangulate_fn=None,
               view_pose_fn=None, two_view_solver: str = "eight-point", two_view_refine: int = 0) -> SceneSeed:
    """A start for target-free bundle adjustment (``FreePointBundleHandler``) from the flat (N, 5) table [cam, im, key, u, v] and the
    intrinsics (C, 9) alone: incremental reconstruction on the device's batched handles.

    1. ``compiled_helpers.estimate_two_view`` on every pair with at least ``min_points`` shared keys.  The first pair is the OK pair
       with the largest n_front * sin(parallax) (many points and a wide baseline; ties: the lower pair).  Its camera a gets the
       identity, its camera b the pair's [R | baseline * t]: the scale of a scene without a target is free, ``baseline`` sets it.
       ``two_view_solver="five-point"`` is for scenes that are mostly one plane (boards, walls, floors), where the eight-point
       hypotheses degenerate; ``two_view_refine`` > 0 refines every pair's pose by that many LM trials at most (``estimate_two_view``'s
       ``solver`` and ``refine_iters``; a ``two_view_fn`` of the caller's receives them only when they differ from the defaults).
    2. Every key that at least two placed cameras see is triangulated and refined (``compiled_helpers.refine_triangulation``;
       ``tri_opts`` reach it, e.g. ``consensus=64``).  While the first pair is alone, only its inliers are triangulated; once a third
       camera is placed every key is, from every placed camera that sees it.
    3. Rounds: every camera not placed yet that sees at least ``min_points`` triangulated keys is resected against them in one batched
       call (``compiled_helpers.estimate_view_poses`` with the triangulated points as template; ``resect_opts`` reach it, e.g.
       ``consensus=64``); a camera whose PnP did not converge stays unplaced.  Then step 2 again.  A round that places nothing ends it.
    4. The world moves to ``ref_cam``'s camera frame; when ``ref_cam`` was not placed it stays with the first pair's camera a
       (``frame_cam`` says which).

    ``two_view_fn``, ``triangulate_fn``, ``view_pose_fn``: replacements with the signatures of the three device entry points."""
    from . import compiled_helpers as ch

    two_view_fn = ch.estimate_two_view if two_view_fn is None else two_view_fn
    triangulate_fn = ch.refine_triangulation if triangulate_fn is None else triangulate_fn
    view_pose_fn = ch.estimate_view_poses if view_pose_fn is None else view_pose_fn
    resect_opts, tri_opts = dict(resect_opts or {}), dict(tri_opts or {})
    d = np.asarray(dct, dtype=np.float64)
    K = np.asarray(intr, dtype=np.float64)
    C = int(n_cams)
    if d.ndim != 2 or d.shape[1] != 5 or K.shape != (C, 9) or C < 2:
        raise ValueError("expected dct (N, 5) = [cam, im, key, u, v] and intr (n_cams, 9) of at least two cameras")
    if isinstance(ref_cam, bool) or not isinstance(ref_cam, (int, np.integer)) or not 0 <= int(ref_cam) < C:
        raise ValueError(f"ref_cam must be a camera index in [0, {C}), got {ref_cam!r}")
    if not (np.isfinite(baseline) and baseline > 0.0):
        raise ValueError(f"baseline must be a finite number > 0, got {baseline!r}")
    ch.check_twoview_options(consensus, inlier_px, seed, min_points)
    ch.check_twoview_solver(two_view_solver, two_view_refine)
    solver_opts = {} if (two_view_solver, int(two_view_refine)) == ("eight-point", 0) else {"solver": two_view_solver, "refine_iters": int(two_view_refine)}
    if not np.all(np.isfinite(d)) or (d.shape[0] and (d[:, 0].min() < 0 or d[:, 0].max() >= C or d[:, 2].min() < 0)):
        raise ValueError("the table must be finite, with cameras inside the intrinsics and keys >= 0")
    n_keys = int(d[:, 2].max()) + 1 if d.shape[0] else 0
    tv = two_view_fn(d, K, consensus=consensus, inlier_px=inlier_px, seed=seed, min_points=min_points, **solver_opts)
    with np.errstate(invalid="ignore"):
        quality = np.where(tv.status == ch.TWOVIEW_OK, tv.n_front * np.sin(tv.parallax), -np.inf)
    if quality.shape[0] == 0 or not np.max(quality) > 0.0:
        raise ValueError("no camera pair has a relative pose: too few shared keys, or only degenerate pairs (coplanar points, no baseline)")
    p0 = int(np.argmax(quality))
    a, b = (int(c) for c in tv.pairs[p0])
    M = np.full((C, 4, 4), np.nan)
    M[a] = np.eye(4)
    M[b] = np.eye(4)
    M[b, :3, :3], M[b, :3, 3] = tv.T[p0, :, :3], float(baseline) * tv.T[p0, :, 3]
    placed = np.zeros(C, dtype=bool)
    placed[[a, b]] = True
    round_of = np.full(C, -1, dtype=np.int64)
    round_of[[a, b]] = 0
    seen = ch.shared_keys(d, C)
    rows0 = slice(int(tv.start[p0]), int(tv.start[p0 + 1]))
    dropped = tv.keys[rows0][~tv.inliers[rows0]]
    pair_only = list(seen)   # what the first triangulation sees: the pair's correspondences without its outliers
    for c in (a, b):
        keep = ~np.isin(seen[c][0], dropped)
        pair_only[c] = (seen[c][0][keep], seen[c][1][keep])
    rnd = 0
    while True:
        points, n_views, rms = _triangulate_placed(pair_only if rnd == 0 else seen, M, K, placed, n_keys, triangulate_fn, tri_opts)
        have = np.all(np.isfinite(points), axis=1)
        cand = [c for c in range(C) if not placed[c] and int(np.sum(have[seen[c][0]])) >= min_points]
        if not cand:
            break
        table = np.concatenate([np.column_stack([np.full(int(np.sum(have[seen[c][0]])), c, dtype=np.float64), np.zeros(int(np.sum(have[seen[c][0]]))),
                                                 seen[c][0][have[seen[c][0]]], seen[c][1][have[seen[c][0]]]]) for c in cand])
        vp = view_pose_fn(table, np.where(have[:, None], points, 0.0), K, n_imgs=1, min_points=min_points, **resect_opts)
        poses, status = np.asarray(vp.poses).reshape(C, 6), np.asarray(vp.status).reshape(C)
        new = [c for c in cand if status[c] == ch.PNP_CONVERGED and np.all(np.isfinite(poses[c]))]
        if not new:
            break
        rnd += 1
        M[new] = pose_to_4x4(poses[new])
        placed[new], round_of[new] = True, rnd
    frame = int(ref_cam) if placed[ref_cam] else a
    if frame != a:
        F = M[frame].copy()
        M = np.where(placed[:, None, None], M @ rigid_inverse(F), np.nan)
        points = points @ F[:3, :3].T + F[:3, 3]
    M[frame] = np.eye(4)
    return SceneSeed(extr=pose_from_4x4(M), points=points, placed=placed, round_of_camera=round_of, n_views=n_views, rms=rms, first_pair=(a, b),
                     frame_cam=frame, two_view=tv)


def align_scene(seed: SceneSeed, reference_points, *, model: str = "similarity", **opts) -> SceneSeed:
    """Bring a seeded scene into the frame and scale of a few known points: ``reference_points`` (K, 3) holds the surveyed position of
    every key that has one and NaN elsewhere.  One registration on the device (``compiled_helpers.align_points``; ``opts`` are its
    options, e.g. ``consensus=64, inlier_dist=...`` against wrong control points) gives X' = s R X + t over the keys that are both
    triangulated and known; the points move to X' and every placed camera gets R_c' = R_c R', t_c' = s t_c - R_c' t, so that a point
    in a camera's frame is s times what it was and every reprojection stays where it is.  ``model="rigid"`` keeps the seed's scale
    (s = 1).  ``frame_cam`` becomes -1: the world is no camera's frame any more.  ValueError when the registration is refused
    (fewer than ``min_points`` common keys, collinear control points); the ``Alignment`` is kept on the result as ``alignment``."""
    from dataclasses import replace

    from . import compiled_helpers as ch

    ref = np.asarray(reference_points, dtype=np.float64)
    pts = np.asarray(seed.points, dtype=np.float64)
    if ref.ndim != 2 or ref.shape[1] != 3 or ref.shape[0] > pts.shape[0]:
        raise ValueError(f"expected reference_points (K, 3) with K <= {pts.shape[0]} keys, NaN where unknown")
    full = np.full_like(pts, np.nan)
    full[: ref.shape[0]] = ref
    al = ch.align_points(pts, full, model=model, **opts)
    if al.status[0] != ch.ALIGN_OK:
        names = {ch.ALIGN_TOO_FEW: "too few keys are both triangulated and known", ch.ALIGN_DEGENERATE: "the control points are collinear",
                 ch.ALIGN_NONFINITE: "no key is both triangulated and known", ch.ALIGN_NO_CONSENSUS: "too few control points agree"}
        raise ValueError(f"align_scene: {names[int(al.status[0])]} ({int(al.n_used[0])} rows used)")
    s, R, t = float(al.scale[0]), al.R[0], al.t[0]
    M = pose_to_4x4(seed.extr)
    placed = np.asarray(seed.placed, dtype=bool)
    Rc = M[:, :3, :3] @ R.T
    M[:, :3, 3] = s * M[:, :3, 3] - Rc @ t
    M[:, :3, :3] = Rc
    extr = np.where(placed[:, None], pose_from_4x4(np.where(placed[:, None, None], M, np.nan)), np.nan)
    out = replace(seed, extr=extr, points=s * pts @ R.T + t, frame_cam=-1)
    out.alignment = al
    return out
